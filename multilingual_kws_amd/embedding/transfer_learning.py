"""Drop-in for multilingual_kws/embedding/transfer_learning.py on MI355X.

transfer_learn() keeps the reference's signature and return contract (name, model, details)
(reference :14-123): a frozen embedding (everything up to "dense_2") with a fresh
Dense(18,tanh) -> Dense(3,softmax) head trained with Adam on freshly augmented batches.
Each step runs augmentation -> micro-frontend -> EfficientNet-B0 forward -> head fwd/bwd/Adam as HIP
kernels; under torch.distributed the batch is sharded across ranks and the head gradient is
all-reduced over RCCL (multilingual_kws_amd/parallel.py).  The frozen phase's trainers, for one head and for K side by side,
sit on one core (_FrozenPhase); the un-frozen phase runs embedding_trainer's tape (on op_tape.OpTape).
"""
import csv
import glob
import json
import os
from typing import Dict, List, Optional

import numpy as np

from .. import parallel, weights
from ..embedding_model import EmbeddingModel
from ..head import Head, HeadGroup, glorot_uniform_params
from . import input_data

CATEGORIES = 3   # silence + unknown + target keyword


def load_base_model(base_model_path, max_batch=1024, base_model_output="dense_2"):
    """The frozen embedding model.  base_model_path: what the reference passes to tf.keras.models.load_model
    (transfer_learning.py:36) -- a Keras SavedModel directory such as multilingual_context_73_0.8011, read without
    TensorFlow by multilingual_kws_amd.checkpoint_import -- or a Keras `.h5` file (model.save / save_weights; read by the same module's
    pure-Python HDF5 reader) -- or a weight-container directory written by
    multilingual_kws_amd.weights.save() (flat float32 blob + manifest with Keras variable names), or
    "synthetic[:SEED]" for the seeded random weights used by benchmarks."""
    p = str(base_model_path)
    if p.startswith("synthetic"):
        seed = int(p.split(":")[1]) if ":" in p else weights.DEFAULT_SEED
        blob = weights.synthetic_blob(seed)
    elif os.path.exists(os.path.join(p, "variables", "variables.index")):
        from .. import checkpoint_import
        blob = checkpoint_import.import_savedmodel(p)
    elif os.path.isfile(p) and p.lower().endswith((".h5", ".hdf5", ".keras.h5")):
        from .. import checkpoint_import                # the other format tf.keras.models.load_model takes: read without libhdf5
        blob = checkpoint_import.import_h5(p)
    else:
        blob = weights.load(p)
    return EmbeddingModel(blob, max_batch=max_batch, output=base_model_output), blob


class TransferLearnedModel:
    """What transfer_learn returns as `model`: frozen embedding + few-shot head with the two Keras
    methods the reference's callers use: predict (run.py, evaluate_files_*) and save (run.py:300)."""

    name = "TransferLearnedModel"

    def __init__(self, embedding, head, blob=None, base_model_path=None):
        self.embedding, self.head = embedding, head
        self._blob, self.base_model_path = blob, base_model_path
        self.history = None

    def predict_device(self, spec):
        """CUDA [N,49,40(,1)] -> CUDA [N,3] class probabilities."""
        import torch
        outs = []
        for s in range(0, spec.shape[0], self.embedding.max_batch):
            outs.append(self.head.forward(self.embedding.forward(spec[s:s + self.embedding.max_batch])))
        return torch.cat(outs) if outs else torch.empty((0, self.head.classes), device=self.embedding.device)

    def predict(self, x, batch_size=None, verbose=0):
        """numpy [N,49,40,1] (or [N,49,40]) -> numpy [N,3]."""
        import torch
        x = torch.as_tensor(np.asarray(x, dtype=np.float32)).to(self.embedding.device)
        if x.dim() == 4:
            x = x[..., 0]
        # checked(): a failed in-kernel exchange poisons the forward that ran it and is otherwise reported by the NEXT call (include/mkws.h);
        # the copy to the host has synchronised anyway, so the host API looks at the handle now and never returns the poisoned batch
        return self.embedding.checked(lambda: self.predict_device(x).cpu().numpy())

    def score(self, x, y=None, batch_size=32):
        """The point scores of the model over a ClipDataset (eval_with_silence_unknown(...).batch(32)) or an array [N,49,40(,1)] with
        labels y: scoring.Scorer.result() -- loss, accuracy, rows, confusion_matrix -- tallied on the device, one copy at the end."""
        from .. import scoring
        return scoring.score_model(self.predict_device, self.embedding.device, self.head.classes, 0, x, y, batch_size, self.embedding.checked)

    def evaluate(self, x, y=None, batch_size=32, verbose=0, return_dict=False):
        """Keras' model.evaluate for a model compiled with sparse categorical cross-entropy on probabilities and metrics=["accuracy"]:
        [loss, accuracy], or {"loss", "accuracy"} with return_dict."""
        from .. import scoring
        return scoring.keras_metrics(self.score(x, y, batch_size), ("loss", "accuracy"), return_dict)

    def save(self, path):
        """Directory with head.npz (+ a copy of / pointer to the base weights)."""
        os.makedirs(path, exist_ok=True)
        np.savez(os.path.join(path, "head.npz"), params=self.head.get_params(),
                 dims=np.asarray([self.head.in_dim, self.head.hidden, self.head.classes]))
        meta = {"format": "mkws-transfer-learned-v1", "base_model_path": self.base_model_path, "base_model_output": self.embedding.output}
        if self._blob is not None and not str(self.base_model_path).startswith("synthetic"):
            weights.save(os.path.join(path, "base"), self._blob)
            meta["base_model_path"] = "base"
        with open(os.path.join(path, "model.json"), "w") as f:
            json.dump(meta, f)

    @classmethod
    def load(cls, path, max_batch=1024):
        meta = json.load(open(os.path.join(path, "model.json")))
        base = meta["base_model_path"]
        if not str(base).startswith("synthetic") and not os.path.isabs(base):
            base = os.path.join(path, base)
        emb, blob = load_base_model(base, max_batch, meta.get("base_model_output", "dense_2"))
        z = np.load(os.path.join(path, "head.npz"))
        i, h, c = [int(v) for v in z["dims"]]
        return cls(emb, Head(i, h, c, max_batch=max_batch, params=z["params"]), blob, meta["base_model_path"])


def load_models_shared(model_paths, max_batch=1024):
    """[TransferLearnedModel.save() directories] -> [TransferLearnedModel] that share ONE embedding handle wherever their base weights are
    the same bytes (the usual case: N few-shot heads on one multilingual embedding, run.py's `modelpaths`).  Models with other base
    weights get their own handle.  Multi-keyword serving (batch_streaming_analysis.streaming_inferences / multi_keyword_detections)
    runs one embedding pass per distinct handle."""
    import hashlib
    shared, out = {}, []
    for path in model_paths:
        path = os.fspath(path)
        meta = json.load(open(os.path.join(path, "model.json")))
        base = meta["base_model_path"]
        if not str(base).startswith("synthetic") and not os.path.isabs(base):
            base = os.path.join(path, base)
        cut = meta.get("base_model_output", "dense_2")
        if str(base).startswith("synthetic"):
            key = (str(base), cut)
        else:       # content, not location: every saved model carries its own copy of the base weights
            h = hashlib.sha256()
            if os.path.isdir(base):                 # SavedModel directory / blob directory
                kind = "dir"
                for root, _, files in sorted(os.walk(base)):
                    for f in sorted(files):
                        h.update(os.path.relpath(os.path.join(root, f), base).encode())
                        h.update(open(os.path.join(root, f), "rb").read())
            elif os.path.isfile(base):              # a Keras .h5 / .npy blob named by model.json (models saved without a blob of their own)
                kind = "file"
                h.update(open(base, "rb").read())
            else:
                raise FileNotFoundError(f"{path}: base model '{base}' (model.json: base_model_path) does not exist")
            key = (kind, h.hexdigest(), cut)
        if key not in shared:
            shared[key] = load_base_model(base, max_batch, cut)
        emb, blob = shared[key]
        z = np.load(os.path.join(path, "head.npz"))
        i, h_, c = [int(v) for v in z["dims"]]
        out.append(TransferLearnedModel(emb, Head(i, h_, c, max_batch=max_batch, params=z["params"], device=emb.device), blob, meta["base_model_path"]))
    return out


FORWARD_CLIPS = 3072     # clips per embedding forward of the frozen phase.  Measured on one MI355X, 512 clips per optimizer step, same calls
                         # (profiles/r05_notes.md section 6): 512 clips per forward (a forward per step) 0.74 ms per step; 1024: 0.58; 2048: 0.548; 3072: 0.534;
                         # 4096: 0.536 (whole multiples of the 1024-clip plan: its workgroup loops run several rounds per launch -- fewer launch
                         # boundaries and tails per clip; 1536 / 2560 clips, a partial last round, are slower than 1024 / 2048)
OVERLAP_FROM_GROUP = 4   # optimizer steps on a second stream from this many steps per forward: +3-4 % at 4 / 6 / 8 steps, -1 % at 2


def steps_per_forward(batch_size, forward_clips=None):
    """Optimizer steps whose batches share one forward pass of the frozen embedding."""
    return max(1, int(FORWARD_CLIPS if forward_clips is None else forward_clips) // max(int(batch_size), 1))


class _FrozenPhase:
    """What the trainers of the frozen phase share (FrozenHeadTrainer, FrozenHeadGroupTrainer): G optimizer steps per forward pass with the
    group_limit cut, the optional second stream for the optimizer steps, `nbuf` alternating embedding buffers and the events that order
    their producer (the caller's stream: `ready`) and consumer (the optimizer stream: `consumed`).  A subclass says how a group is drawn and
    embedded (_refill, between _begin_refill and _hand_over) and what one optimizer step is (_step)."""

    def __init__(self, embedding, batch_size, lr, group, overlap, lead=()):
        """lead: leading dimensions of the embedding buffers [*lead, G * batch_size, features]."""
        import torch
        self.embedding, self.lr, self.bs, self.device = embedding, lr, int(batch_size), embedding.device
        self.G = max(1, min(int(group) if group is not None else steps_per_forward(self.bs), embedding.max_batch // self.bs))
        self.overlap = (self.G >= OVERLAP_FROM_GROUP) if overlap is None else bool(overlap)
        self.side = torch.cuda.Stream(device=self.device) if self.overlap else None
        nbuf = 2 if self.overlap else 1
        self.emb = [torch.empty((*lead, self.G * self.bs, embedding.output_dim), dtype=torch.float32, device=self.device) for _ in range(nbuf)]
        self.consumed = [None] * nbuf            # event: every optimizer step that reads buffer k has run
        self.k, self.j, self.g = -1, 0, 0
        self.forwards = 0

    def _begin_refill(self):
        """The next buffer, once the steps of two groups ago have finished with it: called in front of the first launch that writes it (the
        draws and the launches that make the spectrograms do not wait)."""
        import torch
        self.k = (self.k + 1) % len(self.emb)
        if self.consumed[self.k] is not None:
            torch.cuda.current_stream(self.device).wait_event(self.consumed[self.k])

    def _hand_over(self, g):
        """The group of g steps in buffer k is complete on the caller's stream: the optimizer stream may read it."""
        import torch
        if self.overlap:
            ready = torch.cuda.Event()
            ready.record(torch.cuda.current_stream(self.device))
            self.side.wait_event(ready)
        self.g, self.j = g, 0

    def step(self, group_limit=None):
        """One optimizer step.  group_limit: steps left before the caller needs the head(s) (end of an epoch): a new group is cut to it."""
        import torch
        if self.j >= self.g:
            self._refill(self.G if group_limit is None else max(1, min(self.G, int(group_limit))))
        off = self.j * self.bs
        self.j += 1
        if not self.overlap:
            return self._step(off)
        with torch.cuda.stream(self.side):
            stats = self._step(off)
            if self.j >= self.g:
                ev = self.consumed[self.k] = self.consumed[self.k] or torch.cuda.Event()
                ev.record(self.side)
        return stats

    def accumulate(self, acc, stats):
        """acc += stats on the stream the optimizer steps run on (the statistics tensor is rewritten by the next step)."""
        import torch
        if self.overlap:
            with torch.cuda.stream(self.side):
                acc += stats.to(acc.dtype)
        else:
            acc += stats.to(acc.dtype)

    def finish(self):
        """The caller's stream waits for every optimizer step issued so far."""
        import torch
        if self.overlap:
            torch.cuda.current_stream(self.device).wait_stream(self.side)


class FrozenHeadTrainer(_FrozenPhase):
    """The first phase of transfer_learn (reference transfer_learning.py:38-93: `embedding.trainable = False`, head fitted with Adam)
    as a stream of optimizer steps that does not pay for small forward passes.

    The embedding is frozen, so the forward pass of batch t + 1 is independent of the head update of step t.  G = steps_per_forward
    consecutive batches are therefore drawn together (input_data.BatchGroups: the same draws in the same order as one batch at a time),
    augmented / featurised / SpecAugmented by ONE launch each and embedded by ONE forward pass over G * batch_size clips on a handle
    planned for that size; then the G optimizer steps run one after the other, each on its own batch_size rows and with its own
    all-reduce under torch.distributed -- the semantics of parallel.dp_step, unchanged.  With overlap=True the optimizer steps (a few
    small launches each, nowhere near filling the chip) go to a second stream and run under the NEXT group's augmentation, frontend and
    embedding kernels; two embedding buffers alternate, events order producer and consumer (_FrozenPhase).  Measured on one MI355X at 512
    clips per step (profiles/r05_notes.md): with two steps per forward the second stream loses 1 % (853.9 k -> 844.2 k clips/s: the head's
    few launches only take turns with the embedding's), from four steps per forward it gains 3-4 % (932 k -> 966 k at 4, 958 k -> 984 k at
    6): overlap=None switches it on from OVERLAP_FROM_GROUP steps per forward.  Results are bit-identical either way.

    step() performs exactly one optimizer step and returns its [sum of row losses, #correct] (summed over ranks) as a device tensor
    that is rewritten by the next step() and lives on the trainer's stream: add it up with accumulate(), or read it after finish()
    (which joins the side stream; call it before reading head parameters elsewhere)."""

    def __init__(self, embedding, head, train_ds, batch_size, lr, group=None, overlap=None):
        self.head = head
        self.groups = train_ds if isinstance(train_ds, input_data.BatchGroups) else input_data.BatchGroups(train_ds)
        if self.groups.bs != int(batch_size):
            raise ValueError(f"dataset is batched by {self.groups.bs}, trainer by {int(batch_size)}")
        _FrozenPhase.__init__(self, embedding, batch_size, lr, group, overlap)
        self.cur = None

    def _refill(self, g):
        """Next group of g batches: draws + one launch chain on the caller's stream, hand-over to the optimizer stream."""
        import torch
        spec, labels = self.groups.take(g)
        labels = labels.to(torch.int32)
        self._begin_refill()
        emb = self.embedding.forward(spec, out=self.emb[self.k][:g * self.bs])
        self.forwards += 1
        self._hand_over(g)
        if self.overlap:
            labels.record_stream(self.side)
        self.cur = (emb, labels)

    def _step(self, off):
        emb, labels = self.cur
        return parallel.dp_step(self.head, emb[off:off + self.bs], labels[off:off + self.bs], lr=self.lr)


class FrozenHeadGroupTrainer(_FrozenPhase):
    """FrozenHeadTrainer for K keyword heads side by side on ONE frozen embedding (single process).

    Heads of different keywords are independent, so step j of all K of them is one set of launches with the head as a grid dimension
    (head.HeadGroup) instead of K times four small dependent ones.  Per group of g steps: every target draws its own g batches from
    its own BatchGroups (its own AudioDataset and generator: the draws of transfer_learn), one forward pass per target writes slab k
    of a [K, G * bs, features] buffer, then g rounds of HeadGroup.loss_grad(offset=j * bs, rows=bs) + adam_step.  group_limit, the
    second stream with two alternating buffers and the consumed / ready events are _FrozenPhase's, as for FrozenHeadTrainer.  Every head
    ends with the bits FrozenHeadTrainer gives it alone.

    step() performs one optimizer step of EVERY head and returns a [K, 2] device tensor of their {sum of row losses, #correct}, rewritten
    by the next step()."""

    def __init__(self, embedding, heads, train_dss, batch_size, lr, group=None, overlap=None):
        import torch
        self.group = heads if isinstance(heads, HeadGroup) else HeadGroup(heads)
        self.K = len(self.group)
        self.groups = [d if isinstance(d, input_data.BatchGroups) else input_data.BatchGroups(d) for d in train_dss]
        if len(self.groups) != self.K:
            raise ValueError(f"{self.K} heads but {len(self.groups)} training streams")
        for g in self.groups:
            if g.bs != int(batch_size):
                raise ValueError(f"dataset is batched by {g.bs}, trainer by {int(batch_size)}")
        _FrozenPhase.__init__(self, embedding, batch_size, lr, group, overlap, lead=(self.K,))
        self.labels = [torch.zeros(e.shape[:2], dtype=torch.int32, device=self.device) for e in self.emb]

    def _refill(self, g):
        """Next group of g batches of every target: draws + launch chains on the caller's stream, hand-over to the optimizer stream."""
        n = g * self.bs
        for h, groups in enumerate(self.groups):
            spec, labels = groups.take(g)
            if h == 0:
                self._begin_refill()
            self.embedding.forward(spec, out=self.emb[self.k][h, :n])
            self.labels[self.k][h, :n].copy_(labels)         # int64 -> int32
            self.forwards += 1
        self._hand_over(g)

    def _step(self, off):
        stats = self.group.loss_grad(self.emb[self.k], self.labels[self.k], rows=self.bs, offset=off)
        self.group.adam_step(lr=self.lr)
        return stats

    def close(self):
        """Joins the side stream and drops the group object; the heads stay."""
        import torch
        if self.overlap:
            self.side.synchronize()
        torch.cuda.current_stream(self.device).synchronize()
        self.group.close()


SIDE_BY_SIDE = 8         # heads trained side by side by transfer_learn_many when side_by_side is None (profiles/finetune_many.txt)


def _per_target(what, value, targets):
    """A sequence aligned with `targets`, or a dict keyed by target -> list aligned with targets."""
    if isinstance(value, dict):
        missing = [t for t in targets if t not in value]
        if missing:
            raise ValueError(f"{what} has no entry for target(s) {missing}")
        return [value[t] for t in targets]
    if isinstance(value, (str, bytes)) or not hasattr(value, "__len__"):
        raise ValueError(f"{what} must hold one entry per target (a sequence aligned with targets, or a dict keyed by target)")
    if len(value) != len(targets):
        raise ValueError(f"{what} has {len(value)} entries for {len(targets)} targets")
    return list(value)


def transfer_learn_many(
    targets,
    train_files,
    val_files,
    unknown_files,
    num_epochs,
    num_batches,
    batch_size,
    primary_lr,
    model_settings: Dict,
    base_model_path: os.PathLike,
    base_model_output: str = "dense_2",
    UNKNOWN_PERCENTAGE: float = 50.0,
    bg_datadir: os.PathLike = "/home/mark/tinyspeech_harvard/speech_commands/_background_noise_/",
    csvlog_dest=None,
    verbose=1,
    seed=None,
    side_by_side=None,
    convert=False,
):
    """transfer_learn for several target keywords on ONE frozen embedding, their heads trained side by side.

    train_files / val_files: one list per target (a sequence aligned with `targets`, or a dict keyed by target); unknown_files and
    bg_datadir are shared.  seed: None, an int (target i gets seed + i) or one seed per target; csvlog_dest: None or one path per target.
    Returns [(name, model, details)] in target order, each entry with transfer_learn's contract, and for the same seed the same bits
    as transfer_learn(target, ..., backprop_into_embedding=False, seed=seed_i) returns; all models share one EmbeddingModel (as
    load_models_shared's do), so Head.forward_many / streaming_inferences take them as they are.

    side_by_side heads (default SIDE_BY_SIDE, at most len(targets)) advance together: per group of steps one forward pass per target,
    then every optimizer step as ONE set of launches for all of them (FrozenHeadGroupTrainer).  More targets run in waves.

    There is no backprop_into_embedding here: that phase trains one embedding per keyword and has nothing to share -- call
    transfer_learn.  Under torch.distributed with more than one rank the targets run one after the other through transfer_learn (same
    results; one collective per optimizer step, as there), and each model has its own embedding handle.
    convert: AudioDataset's switch (clip files and background tracks of any supported format, rate and channel count)."""
    from ..embedding_model import OUTPUT_LAYERS
    targets = list(targets)
    if len(targets) == 0:
        raise ValueError("transfer_learn_many needs at least one target")
    if len(set(targets)) != len(targets):
        raise ValueError(f"duplicate targets: {sorted(t for t in set(targets) if targets.count(t) > 1)}")
    train_files = _per_target("train_files", train_files, targets)
    val_files = _per_target("val_files", val_files, targets)
    if seed is None:
        seeds = [None] * len(targets)
    elif isinstance(seed, (int, np.integer)):
        seeds = [int(seed) + i for i in range(len(targets))]
    else:
        seeds = [None if s is None else int(s) for s in _per_target("seed", seed, targets)]
    csvs = [None] * len(targets) if csvlog_dest is None else _per_target("csvlog_dest", csvlog_dest, targets)
    if base_model_output not in OUTPUT_LAYERS:
        raise ValueError(f"base_model_output {base_model_output!r}: this build cuts the embedding at one of {sorted(OUTPUT_LAYERS)}")
    if side_by_side is not None and int(side_by_side) < 1:
        raise ValueError("side_by_side must be at least 1")
    common = dict(unknown_files=unknown_files, num_epochs=num_epochs, num_batches=num_batches, batch_size=batch_size, primary_lr=primary_lr,
                  model_settings=model_settings, base_model_path=base_model_path, base_model_output=base_model_output,
                  UNKNOWN_PERCENTAGE=UNKNOWN_PERCENTAGE, bg_datadir=bg_datadir, verbose=verbose, convert=convert)
    if parallel.world_size() > 1:
        return [transfer_learn(t, train_files[i], val_files[i], backprop_into_embedding=False, embedding_lr=0, csvlog_dest=csvs[i],
                               seed=seeds[i], **common) for i, t in enumerate(targets)]
    import torch
    wave = min(len(targets), int(side_by_side) if side_by_side is not None else SIDE_BY_SIDE)
    group = steps_per_forward(batch_size)
    embedding, blob = load_base_model(base_model_path, max_batch=max(batch_size * group, 64), base_model_output=base_model_output)
    feat = embedding.output_dim
    steps_per_epoch = batch_size * num_batches          # (sic) -- reference :89
    results, donor = [], None
    for w0 in range(0, len(targets), wave):
        idx = list(range(w0, min(w0 + wave, len(targets))))
        xfers, train_dss, val_dss = [], [], []
        for i in idx:
            head = Head(feat, 18, CATEGORIES, max_batch=max(batch_size, 64), params=glorot_uniform_params(feat, 18, CATEGORIES, seeds[i]),
                        device=embedding.device)
            xfers.append(TransferLearnedModel(embedding, head, blob, str(base_model_path)))
            ds = input_data.AudioDataset(model_settings=model_settings, commands=[targets[i]], background_data_dir=bg_datadir,
                                         unknown_files=unknown_files, unknown_percentage=UNKNOWN_PERCENTAGE,
                                         spec_aug_params=input_data.SpecAugParams(percentage=80), seed=seeds[i], convert=convert)
            if donor is None:
                donor = ds
            else:
                ds.share_banks(donor)       # the unknown bank and the background tracks are decoded and uploaded once, not per target
            tds, vds = _few_shot_datasets(ds, train_files[i], val_files[i], batch_size)
            train_dss.append(tds)
            val_dss.append(vds)
        K = len(idx)
        frozen = FrozenHeadGroupTrainer(embedding, [x.head for x in xfers], train_dss, batch_size, primary_lr, group=group)
        histories = [{"loss": [], "accuracy": [], "val_loss": [], "val_accuracy": []} for _ in idx]
        for epoch in range(num_epochs):
            acc_stats = torch.zeros((K, 2), dtype=torch.float64, device=embedding.device)
            for step_i in range(steps_per_epoch):
                # never across the end of an epoch: validation reads the heads there
                frozen.accumulate(acc_stats, frozen.step(group_limit=steps_per_epoch - step_i))
            frozen.finish()
            train_stats = (acc_stats / max(steps_per_epoch * batch_size, 1)).tolist()
            for k, i in enumerate(idx):
                _end_epoch(histories[k], xfers[k], val_dss[k], train_stats[k][0], train_stats[k][1], epoch, num_epochs, steps_per_epoch, verbose,
                           tag=f"[{targets[i]}] ")
        frozen.close()
        for k, i in enumerate(idx):
            results.append(_finish(xfers[k], histories[k], targets[i], num_epochs, batch_size, num_batches, csvs[i]))
    return results


def _validate(xfer, val_ds):
    """(mean loss, accuracy) of `xfer` over the validation set (every rank evaluates the full, small set)."""
    import torch
    vstats, vseen = np.zeros(2), 0
    for spec, labels in val_ds:
        probs = xfer.predict_device(spec[..., 0])
        lab = labels.long()
        vstats[0] += float(-torch.log(torch.clamp(probs[torch.arange(len(lab)), lab], min=1e-7)).sum())
        vstats[1] += float((probs.argmax(1) == lab).sum())
        vseen += len(lab)
    return (vstats / max(vseen, 1)).tolist()


def _end_epoch(history, xfer, val_ds, tl, ta, epoch, num_epochs, steps_per_epoch, verbose, tag=""):
    """Validation on the current weights, one more entry in every list of `history`, the Keras-style progress line."""
    vl, va = _validate(xfer, val_ds)
    for k, v in zip(("loss", "accuracy", "val_loss", "val_accuracy"), (tl, ta, vl, va)):
        history[k].append(v)
    if verbose:
        print(f"{tag}Epoch {epoch + 1}/{num_epochs} - {steps_per_epoch} steps - loss: {tl:.4f} - accuracy: {ta:.4f} "
              f"- val_loss: {vl:.4f} - val_accuracy: {va:.4f}")


def _finish(xfer, history, target, num_epochs, batch_size, num_batches, csvlog_dest):
    """The tail of a fine-tune: CSV log, model.history, and the reference's (name, model, details)."""
    if csvlog_dest is not None:
        with open(csvlog_dest, "w", newline="") as f:
            w = csv.writer(f)
            w.writerow(["epoch", "accuracy", "loss", "val_accuracy", "val_loss"])
            for e in range(num_epochs):
                w.writerow([e, history["accuracy"][e], history["loss"][e], history["val_accuracy"][e], history["val_loss"][e]])
    xfer.history = history
    va = history["val_accuracy"][-1] if history["val_accuracy"] else 0.0
    name = f"xfer_epochs_{num_epochs}_bs_{batch_size}_nbs_{num_batches}_val_acc_{va:0.2f}_target_{target}"
    details = dict(num_epochs=num_epochs, batch_size=batch_size, num_batches=num_batches, val_accuracy=va, target=target)
    return name, xfer, details


def _few_shot_datasets(audio_dataset, train_files, val_files, batch_size):
    AUTOTUNE = input_data.AUTOTUNE
    init_train_ds = audio_dataset.init_single_target(AUTOTUNE, train_files, is_training=True)
    init_val_ds = audio_dataset.init_single_target(AUTOTUNE, val_files, is_training=False)
    return init_train_ds.shuffle(buffer_size=1000).repeat().batch(batch_size), init_val_ds.batch(batch_size)


def transfer_learn(
    target,
    train_files,
    val_files,
    unknown_files,
    num_epochs,
    num_batches,
    batch_size,
    primary_lr,
    backprop_into_embedding,
    embedding_lr,
    model_settings: Dict,
    base_model_path: os.PathLike,
    base_model_output: str,
    UNKNOWN_PERCENTAGE: float = 50.0,
    bg_datadir: os.PathLike = "/home/mark/tinyspeech_harvard/speech_commands/_background_noise_/",
    csvlog_dest: Optional[os.PathLike] = None,
    verbose=1,
    seed=None,
    convert=False,
):
    """Single-target few-shot fine-tune; see the reference's docstring ("this only works for
    single-target models").  Extra keyword: `seed` (augmentation + head init; rank is added under DP).
    batch_size is the PER-RANK batch under torch.distributed (weak scaling).  convert: AudioDataset's switch."""
    from ..embedding_model import OUTPUT_LAYERS
    if base_model_output not in OUTPUT_LAYERS:       # reference :38-42 cuts at get_layer(name=base_model_output)
        raise ValueError(f"base_model_output {base_model_output!r}: this build cuts the embedding at one of {sorted(OUTPUT_LAYERS)}")
    if backprop_into_embedding and base_model_output != "dense_2":
        raise ValueError('backprop_into_embedding=True is implemented for base_model_output="dense_2" (the only value the reference\'s callers pass)')
    import torch
    rank, world = parallel.rank(), parallel.world_size()
    group = steps_per_forward(batch_size)                # optimizer steps per forward pass of the frozen embedding (FrozenHeadTrainer)
    embedding, blob = load_base_model(base_model_path, max_batch=max(batch_size * group, 64), base_model_output=base_model_output)
    feat = embedding.output_dim
    head_seed = None if seed is None else int(seed)
    p0 = glorot_uniform_params(feat, 18, CATEGORIES, head_seed)
    if world > 1:      # identical initial head on every rank
        t = torch.from_numpy(p0).to(embedding.device)
        parallel.broadcast_(t, 0)
        p0 = t.cpu().numpy()
    head = Head(feat, 18, CATEGORIES, max_batch=max(batch_size, 64), params=p0, device=embedding.device)
    xfer = TransferLearnedModel(embedding, head, blob, str(base_model_path))

    audio_dataset = input_data.AudioDataset(
        model_settings=model_settings,
        commands=[target],
        background_data_dir=bg_datadir,
        unknown_files=unknown_files,
        unknown_percentage=UNKNOWN_PERCENTAGE,
        spec_aug_params=input_data.SpecAugParams(percentage=80),
        seed=None if seed is None else int(seed) + 1000003 * rank,   # decorrelated per-rank streams
        convert=convert,
    )
    train_ds, val_ds = _few_shot_datasets(audio_dataset, train_files, val_files, batch_size)

    steps_per_epoch = batch_size * num_batches          # (sic) -- reference :89
    train_groups = input_data.BatchGroups(train_ds)      # ONE stream of batches for both phases (the draws continue across them)
    frozen = FrozenHeadTrainer(embedding, head, train_groups, batch_size, primary_lr, group=group)
    phases = [("head", primary_lr)]
    if backprop_into_embedding:
        # reference :94-112: `layer.trainable = True` on the nested embedding Model un-freezes ALL of its layers
        # (BatchNormalization too), the model is re-compiled with a fresh Adam(embedding_lr) and fitted again for
        # the same number of epochs; the returned history / val_accuracy are the second fit's.
        phases.append(("all", embedding_lr))
    trainer, history = None, None
    for phase, lr in phases:
        if phase == "all":
            from ..embedding_trainer import EmbeddingTrainer, TrainStepGraph, drop_connect_rates
            trainer, rates = EmbeddingTrainer(blob, device=embedding.device), drop_connect_rates()
            head.reset_optimizer()
            graphed = None          # one hipGraph replay per step (single process; the DP phase keeps the launch-by-launch path)
        history = {"loss": [], "accuracy": [], "val_loss": [], "val_accuracy": []}
        for epoch in range(num_epochs):
            acc_stats = torch.zeros(2, dtype=torch.float64, device=embedding.device)
            seen = 0
            for step_i in range(steps_per_epoch):
                if trainer is None:
                    # frozen embedding: G batches per forward pass, never across the end of an epoch (validation reads the head there)
                    stats = frozen.step(group_limit=steps_per_epoch - step_i)
                    frozen.accumulate(acc_stats, stats)
                    seen += batch_size * world
                    continue
                spec, labels = train_groups.take(1)
                nb = spec.shape[0]
                masks = {name: audio_dataset.rng.uniform(0, 1, nb) >= rate for name, rate in rates.items()}
                if world == 1:
                    if graphed is None or graphed.B != nb:
                        graphed = TrainStepGraph(trainer, head, nb, lr)
                    stats = graphed.run(spec, labels, masks)
                else:
                    emb = trainer.forward_train(spec, masks)
                    stats = head.loss_grad(emb, labels)
                    trainer.backward(head.input_grad(nb), allreduce=world > 1)
                    if world > 1:
                        stats = parallel.allreduce_sum_(head.grad_view(with_stats=True))[-2:]
                    head.adam_step(lr=lr, grad_scale=1.0 / world)
                    trainer.adam_step(lr=lr, grad_scale=1.0 / world)
                acc_stats += stats.to(torch.float64)
                seen += spec.shape[0] * world
            frozen.finish()
            tl, ta = (acc_stats / max(seen, 1)).tolist()
            if trainer is not None:      # validation runs the inference kernels on the current weights (moving statistics)
                blob = trainer.blob()
                embedding = EmbeddingModel(blob, max_batch=max(batch_size, 64), device=embedding.device, output=base_model_output)
                xfer.embedding, xfer._blob = embedding, blob
                xfer.base_model_path = "fine-tuned:" + str(base_model_path)
            _end_epoch(history, xfer, val_ds, tl, ta, epoch, num_epochs, steps_per_epoch, verbose and rank == 0)
    return _finish(xfer, history, target, num_epochs, batch_size, num_batches, csvlog_dest if rank == 0 else None)


def _specs_for_files(files, model_settings, convert=False):
    """file2spec over a list, batched: decode on the host, one frontend launch for all clips.  convert=True: decoded and brought to the
    model's rate on the device instead (input_data.read_clips, channel 0)."""
    import torch
    n = model_settings["desired_samples"]
    if convert and len(files):
        audio = input_data.read_clips(files, model_settings["sample_rate"], n)
        return input_data.to_micro_spectrogram(model_settings, audio).cpu().numpy()
    audio = np.stack([input_data._read_wav(f, n) for f in files]) if len(files) else np.zeros((0, n), np.float32)
    if len(files) == 0:
        return np.zeros((0, model_settings["spectrogram_length"], model_settings["fingerprint_width"]), np.float32)
    return input_data.to_micro_spectrogram(model_settings, torch.from_numpy(audio).cuda()).cpu().numpy()


def _pick(words_to_evaluate, data_dir, utterances_per_word):
    fs_all = []
    for word in words_to_evaluate:
        wavs = glob.glob(data_dir + word + "/*.wav")
        if len(wavs) > utterances_per_word:
            fs = np.random.choice(wavs, utterances_per_word, replace=False)
        else:
            print("using all wavs for ", word)
            fs = wavs
        fs_all.extend(list(fs))
    return fs_all


def _split_confidences(preds, target_id):
    correct, incorrect = [], []
    for row, col in enumerate(np.argmax(preds, axis=1)):
        (correct if col == target_id else incorrect).append(preds[row][col])
    return dict(correct=correct, incorrect=incorrect)


def evaluate_fast_multiclass(words_to_evaluate: List[str], target_id: int, data_dir: os.PathLike,
                             utterances_per_word: int, model, model_settings: Dict):
    specs = _specs_for_files(_pick(words_to_evaluate, data_dir, utterances_per_word), model_settings)
    return _split_confidences(model.predict(np.expand_dims(specs, -1)), target_id)


def evaluate_fast_single_target(words_to_evaluate: List[str], target_id: int, data_dir: os.PathLike,
                                utterances_per_word: int, model, model_settings: Dict):
    specs = _specs_for_files(_pick(words_to_evaluate, data_dir, utterances_per_word), model_settings)
    preds = model.predict(np.expand_dims(specs, -1))
    return preds[:, target_id], preds


def evaluate_files_multiclass(files_to_evaluate: List[os.PathLike], target_id: int, model, model_settings: Dict):
    specs = _specs_for_files(files_to_evaluate, model_settings)
    return _split_confidences(model.predict(np.expand_dims(specs, -1)), target_id)


def evaluate_files_single_target(files_to_evaluate: List[os.PathLike], target_id: int, model, model_settings: Dict):
    """-> (preds[:, target_id], preds) exactly as the reference (:264-273)."""
    specs = _specs_for_files(files_to_evaluate, model_settings)
    preds = model.predict(np.expand_dims(specs, -1))
    return preds[:, target_id], preds


def _shared_embedding(models):
    """The one embedding handle and the heads of `models`; ValueError unless they share it (load_models_shared / transfer_learn_many)."""
    models = list(models)
    if not models:
        raise ValueError("at least one model")
    embedding = models[0].embedding
    if any(m.embedding is not embedding for m in models):
        raise ValueError("the models do not share one embedding handle: load them with load_models_shared, or train them with "
                         "transfer_learn_many")
    heads = [m.head for m in models]
    if len({(h.in_dim, h.hidden, h.classes) for h in heads}) != 1:
        raise ValueError("the models' heads differ in their dimensions")
    return embedding, heads


def evaluate_files_many(files_to_evaluate: List[os.PathLike], models, model_settings: Dict, as_device=False, convert=False):
    """evaluate_files_single_target for K models on one embedding handle: every clip is decoded, featurised and embedded ONCE (in
    batches of the handle's max_batch) and all K heads run in one launch per batch.  -> preds [K, N, classes], numpy or (as_device=True)
    a CUDA tensor; preds[k] has the bits of evaluate_files_single_target(files_to_evaluate, 2, models[k], model_settings)[1].
    convert=True: the files may have any supported format, rate and channel count; each batch is decoded and brought to the model's rate
    on the device (input_data.read_clips, channel 0).  With the default a file is taken as 16-bit PCM at the model's rate."""
    import torch
    embedding, heads = _shared_embedding(models)
    files = [os.fspath(f) for f in files_to_evaluate]
    n_samples, mb = model_settings["desired_samples"], embedding.max_batch
    specs = []                                           # featurised once, whatever happens to the embedding passes below
    with torch.cuda.device(embedding.device):
        for s in range(0, len(files), mb):
            if convert:
                audio = input_data.read_clips(files[s:s + mb], model_settings["sample_rate"], n_samples, device=embedding.device)
                specs.append(input_data.to_micro_spectrogram(model_settings, audio))
                continue
            audio = np.stack([input_data._read_wav(f, n_samples) for f in files[s:s + mb]])
            specs.append(input_data.to_micro_spectrogram(model_settings, torch.from_numpy(audio).to(embedding.device)))

    def run():
        preds = torch.empty((len(heads), len(files), heads[0].classes), dtype=torch.float32, device=embedding.device)
        for i, spec in enumerate(specs):
            preds[:, i * mb:i * mb + spec.shape[0]] = Head.forward_many(heads, embedding.forward(spec))
        if as_device:
            torch.cuda.current_stream(embedding.device).synchronize()     # checked() looks at the handle after the passes have run
            return preds
        return preds.cpu().numpy()

    # the exchange-failure check of TransferLearnedModel.predict: a poisoned batch is never handed back
    return embedding.checked(run)


def keyword_labels(keyword_of_clip, n_keywords):
    """Which keyword every clip says (an id in [0, n_keywords), -1 for silence, anything else -- n_keywords and above -- for a word no
    model spots) -> int32 [n_keywords, N]: model k's label of clip n is 2 where the clip is keyword k, 0 where it is silence, 1
    (unknown) otherwise.  With it one evaluate_many pass yields every keyword's 3 x 3 matrix."""
    ids = np.asarray(keyword_of_clip)
    if ids.ndim != 1 or (ids.size and not np.issubdtype(ids.dtype, np.integer)):
        raise ValueError("keyword_of_clip must be a vector of integer keyword ids")
    if int(n_keywords) < 1:
        raise ValueError(f"n_keywords = {n_keywords}")
    ids = ids.astype(np.int64)
    if ids.size and ids.min() < -1:
        raise ValueError(f"keyword id {int(ids.min())}: -1 is silence, there is no other negative id")
    labels = np.ones((int(n_keywords), ids.size), np.int32)
    labels[:, ids == -1] = 0
    labels[ids[None, :] == np.arange(int(n_keywords))[:, None]] = 2
    return labels


def evaluate_many(models, x, y=None, labels=None, batch_size=1024, return_dict=True):
    """model.evaluate for K few-shot models at once.  Models that share an embedding handle (load_models_shared, transfer_learn_many)
    are scored together: one embedding pass per batch, Head.forward_many to [K, B, 3], one scorer call; models on different handles are
    grouped by handle, as evaluate_files_many's callers group them, and every group makes its own pass over x.
    x: a ClipDataset, or an array [N,49,40(,1)] with labels; labels (or y): [N] shared by the models, or [K, N] per model
    (keyword_labels); with a dataset and labels=None the dataset's own labels are shared.  With labels given for a dataset, they are taken
    in the order the dataset yields its clips.
    -> one {"loss", "accuracy", "rows", "confusion_matrix"} per model (return_dict=False: [loss, accuracy] per model)."""
    import torch
    from .. import scoring
    models = list(models)
    if not models:
        raise ValueError("at least one model")
    if labels is None:
        labels = y
    by_handle = {}
    for k, m in enumerate(models):
        by_handle.setdefault(id(m.embedding), []).append(k)
    is_array = torch.is_tensor(x) or isinstance(x, (np.ndarray, list, tuple))
    if is_array and labels is None:
        raise ValueError("evaluate_many: labels are required when x is an array")
    lab = None if labels is None else np.asarray(labels.cpu() if torch.is_tensor(labels) else labels)
    if lab is not None and (lab.ndim not in (1, 2) or (lab.ndim == 2 and lab.shape[0] != len(models))):
        raise ValueError(f"evaluate_many: labels must be [N] or [{len(models)}, N], got {lab.shape}")
    out = [None] * len(models)
    for ks in by_handle.values():
        embedding, heads = _shared_embedding([models[k] for k in ks])
        scorer = scoring.Scorer(len(ks), heads[0].classes, 0, device=embedding.device)
        d_lab = None
        if lab is not None:
            d_lab = torch.from_numpy(np.ascontiguousarray(lab if lab.ndim == 1 else lab[ks]).astype(np.int32)).to(embedding.device)

        def run():
            scorer.reset()
            at = 0
            batches = scoring.eval_batches(x, torch.zeros(len(x), dtype=torch.int32) if is_array else None, batch_size, embedding.device)
            for spec, own in batches:
                B = int(spec.shape[0])
                for s in range(0, B, embedding.max_batch):
                    e = min(s + embedding.max_batch, B)
                    probs = Head.forward_many(heads, embedding.forward(spec[s:e]))
                    scorer.add(probs, own[s:e] if d_lab is None else d_lab[..., at + s:at + e])
                at += B
            if d_lab is not None and at != d_lab.shape[-1]:
                raise ValueError(f"evaluate_many: {d_lab.shape[-1]} labels for {at} clips")
            return scorer.result()

        res = embedding.checked(run)
        for i, k in enumerate(ks):
            out[k] = (dict(loss=float(res.loss[i]), accuracy=float(res.accuracy[i]), rows=int(res.rows[i]), confusion_matrix=res.confusion_matrix[i])
                      if return_dict else scoring.keras_metrics(res, model=i))
    return out


def classification_curves(models, target_files, unknown_files, model_settings: Optional[Dict] = None, thresholds=None, multiclass=False,
                          convert=False):
    """The classification ROC of K keyword models on one embedding handle (the reference's batch_transfer_learning_analysis.py:114-171
    followed by roc_single_target, one keyword at a time there).  target_files / unknown_files: K lists of WAV paths, model k's target
    clips and its non-target clips; the lists may overlap (one non-target pool for all keywords is the usual case) and a path listed
    twice counts twice.  Every distinct path is embedded once, all heads run in one launch per batch (evaluate_files_many) and the counts
    are taken on the device (transfer_learning_analysis.roc_many): no probability leaves the device.
    -> one dict per keyword: tprs, fprs, threshs (what roc_single_target -- multiclass=True: roc_sc -- returns for that keyword's
    confidences, at `thresholds`, default the reference's 101), n_target, n_unknown.  convert: evaluate_files_many's switch."""
    from .transfer_learning_analysis import roc_many
    models = list(models)
    _shared_embedding(models)
    target_files, unknown_files = [list(x) for x in target_files], [list(x) for x in unknown_files]
    if len(target_files) != len(models) or len(unknown_files) != len(models):
        raise ValueError(f"{len(target_files)} lists of target files and {len(unknown_files)} of unknown files for {len(models)} models")
    if model_settings is None:
        model_settings = input_data.standard_microspeech_model_settings(label_count=3)
    row = {}                                             # distinct paths in first-seen order
    positives = [[row.setdefault(os.fspath(f), len(row)) for f in fs] for fs in target_files]
    negatives = [[row.setdefault(os.fspath(f), len(row)) for f in fs] for fs in unknown_files]
    preds = evaluate_files_many(list(row), models, model_settings, as_device=True, convert=convert)
    curves = roc_many(preds, positives, negatives, thresholds=thresholds, multiclass=multiclass, target_id=2, negative_class=1)
    return [dict(tprs=tprs, fprs=fprs, threshs=threshs, n_target=len(positives[k]), n_unknown=len(negatives[k]))
            for k, (tprs, fprs, threshs) in enumerate(curves)]
