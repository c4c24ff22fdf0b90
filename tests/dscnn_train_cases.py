"""The float64 oracle of one DS-CNN training step, shared by tests/test_dscnn_train_cpu.py and tests/test_dscnn_train_gpu.py.

A torch restatement on UNFOLDED parameters with autograd: explicit SAME padding, BatchNorm on batch statistics with Keras' moving-average
update (conv biases included, as Keras has them), the dropout masks passed in as arrays, the pool over rows 0..23, dense, log-softmax
and cross-entropy, L2 on the nine convolution kernels, Keras Adam.  Inputs are dscnn.structured_clips and dscnn.synthetic_params
(non-trivial BatchNorm, non-zero conv biases), as in tests/dscnn_cases.py."""
import functools

import numpy as np
import torch

from multilingual_kws_amd import dscnn, dscnn_trainer

F = torch.nn.functional
LABELS = 7
PARAM_SEED, CLIP_SEED = 1234, 4242
EPS = float(np.float32(1e-3))
MOMENTUM = 0.99
TRAINABLE_LEAVES = ("kernel", "depthwise_kernel", "bias", "gamma", "beta")
LAYERS = dscnn_trainer.LAYERS
CONV_KERNELS, CONV_BIASES = dscnn_trainer.CONV_KERNELS, dscnn_trainer.CONV_BIASES


@functools.lru_cache(maxsize=None)
def params(label_count=LABELS):
    p = dscnn.synthetic_params(label_count, PARAM_SEED)
    p.setflags(write=False)
    return p


@functools.lru_cache(maxsize=None)
def clips(n, seed=CLIP_SEED):
    x = dscnn.structured_clips(n, seed)
    x.setflags(write=False)
    return x


def labels_for(n, label_count=LABELS):
    """n labels that cover min(n, label_count) classes (at least 3 from n = 3 on)."""
    return ((np.arange(n) * 3 + 1) % label_count).astype(np.int32)


def trainable(name):
    return name.split("/")[1] in TRAINABLE_LEAVES


def tensors64(blob):
    """blob -> {name: float64 copy}"""
    return {n: v.astype(np.float64) for n, v in dscnn.unpack(np.asarray(blob, dtype=np.float32)).items()}


def to_blob(named, label_count):
    blob = np.zeros(dscnn.param_count(label_count), np.float32)
    for n, v in dscnn.unpack(blob).items():
        v[...] = np.asarray(named[n], dtype=np.float64).reshape(v.shape)
    return blob


def host_masks(seed, step, B, rates=(0.2, 0.4)):
    """The two dropout masks of step `step` as float64 [B,25,20,64] arrays, already scaled by the float32 1 / (1 - rate)."""
    n = B * 25 * 20 * 64
    return [dscnn_trainer.dropout_mask_host(seed, step, site, n, rate).reshape(B, 25, 20, 64).astype(np.float64) * float(dscnn_trainer.dropout_scale(rate))
            for site, rate in ((dscnn_trainer.SITE_STEM, rates[0]), (dscnn_trainer.SITE_POOL, rates[1]))]


def _bn(z, t, prefix, training, out):
    """z [B,C,H,W]"""
    g, b = t[prefix + "/gamma"].view(1, -1, 1, 1), t[prefix + "/beta"].view(1, -1, 1, 1)
    if training:
        M = z.shape[0] * z.shape[2] * z.shape[3]
        mean, var = z.mean(dim=(0, 2, 3)), z.var(dim=(0, 2, 3), unbiased=False)
        out["batch"][prefix] = (mean.detach().numpy().copy(), var.detach().numpy().copy())
        out["moving"][prefix + "/moving_mean"] = (MOMENTUM * t[prefix + "/moving_mean"] + (1 - MOMENTUM) * mean).detach().numpy()
        out["moving"][prefix + "/moving_variance"] = (MOMENTUM * t[prefix + "/moving_variance"] + (1 - MOMENTUM) * var * (M / (M - 1))).detach().numpy()
    else:
        mean, var = t[prefix + "/moving_mean"], t[prefix + "/moving_variance"]
    return (z - mean.view(1, -1, 1, 1)) / torch.sqrt(var.view(1, -1, 1, 1) + EPS) * g + b


KINK = 1e-5         # |pre-activation| (in units of the BatchNorm output, scale about 1) up to which float32 may land on the other side of a ReLU


def forward(named, spec, masks=None, training=True, alive=None, signs=None):
    """named {name: float64 array or tensor}, spec [B,49,40], masks None or [stem mask, pool mask] ([B,25,20,64], scaled) ->
    (logits [B,L] tensor, dict(batch, moving)).  alive (a list) receives every ReLU's share of positive outputs.
    signs: None, or per layer a bool [B,25,20,64] (or None) saying on which side of its ReLU another computation found each
    pre-activation.  Where the oracle's own pre-activation is within KINK of zero -- where a float32 forward pass may legitimately be
    on either side, and where 0 and 1 are both subgradients of the ReLU at the limit -- that side is taken; out["kinks"] counts those
    cells per layer and out["flipped"] the cells FARTHER than KINK from zero whose given side differs from the oracle's (none, for a
    correct forward pass)."""
    t = {n: (v if torch.is_tensor(v) else torch.from_numpy(np.asarray(v, dtype=np.float64))) for n, v in named.items()}
    out = dict(batch={}, moving={}, kinks=[], flipped=[])
    x = torch.from_numpy(np.asarray(spec, dtype=np.float64))[:, None]
    x = F.pad(x, (1, 1, 4, 5))                                 # SAME for 10x4 stride 2: left 1, right 1, top 4, bottom 5
    for i, (kind, kernel, bias, prefix) in enumerate(LAYERS):
        w = t[kernel]
        if kind == "stem":
            z = F.conv2d(x, w.permute(3, 2, 0, 1), stride=2)
        elif kind == "dw":
            z = F.conv2d(x, w.permute(2, 3, 0, 1), padding=1, groups=64)
        else:
            z = F.conv2d(x, w.permute(3, 2, 0, 1))
        z = z + t[bias].view(1, -1, 1, 1)
        y = _bn(z, t, prefix, training, out)
        if signs is not None and signs[i] is not None:
            theirs, mine, near = torch.from_numpy(signs[i]).permute(0, 3, 1, 2), y.detach() > 0, y.detach().abs() <= KINK
            out["kinks"].append(int((near & (theirs != mine)).sum()))
            out["flipped"].append(int((~near & (theirs != mine)).sum()))
            x = y * torch.where(near, theirs, mine)
        else:
            x = torch.relu(y)
        if alive is not None:
            alive.append(float((x > 0).double().mean()))
        if i == 0 and masks is not None:
            x = x * torch.from_numpy(masks[0]).permute(0, 3, 1, 2)
    if masks is not None:
        x = x * torch.from_numpy(masks[1]).permute(0, 3, 1, 2)
    pooled = x[:, :, :dscnn.POOL_ROWS, :].mean(dim=(2, 3))
    return pooled @ t["dense/kernel"] + t["dense/bias"], out


def regularization(t, weight_decay):
    return weight_decay * sum((t[k] ** 2).sum() for k in CONV_KERNELS)


def step(named, spec, labels, masks=None, weight_decay=0.0, signs=None):
    """One training-mode forward + backward -> dict(loss (mean cross-entropy, without L2), loss_sum, correct, grads {trainable name:
    array}, batch {prefix: (mean, var)}, moving {name: updated array}, logits, kinks, flipped); signs as in forward()."""
    t = {n: torch.from_numpy(np.asarray(v, dtype=np.float64).copy()).requires_grad_(trainable(n)) for n, v in named.items()}
    logits, out = forward(t, spec, masks, training=True, signs=signs)
    y = torch.from_numpy(np.asarray(labels, dtype=np.int64))
    rows = -torch.log_softmax(logits, dim=1)[torch.arange(len(y)), y]
    total = rows.mean() + regularization(t, weight_decay)
    total.backward()
    out.update(loss=float(rows.mean().detach()), loss_sum=float(rows.sum().detach()), correct=int((logits.argmax(dim=1) == y).sum()), logits=logits.detach().numpy(),
               grads={n: v.grad.numpy() for n, v in t.items() if trainable(n)})
    return out


def loss_only(named, spec, labels, masks=None, weight_decay=0.0):
    with torch.no_grad():
        t = {n: torch.from_numpy(np.asarray(v, dtype=np.float64)) for n, v in named.items()}
        logits, _ = forward(t, spec, masks, training=True)
        y = torch.from_numpy(np.asarray(labels, dtype=np.int64))
        return float((-torch.log_softmax(logits, dim=1)[torch.arange(len(y)), y]).mean() + regularization(t, weight_decay))


def eval_logits(named, spec):
    with torch.no_grad():
        return forward(named, spec, None, training=False)[0].numpy()


def adam(p, g, m, v, t, lr, beta1=0.9, beta2=0.999, eps=1e-7):
    """Keras Adam, float64: step index t >= 1 -> (p, m, v)."""
    m = beta1 * m + (1 - beta1) * g
    v = beta2 * v + (1 - beta2) * g * g
    lr_t = lr * np.sqrt(1 - beta2 ** t) / (1 - beta1 ** t)
    return p - lr_t * m / (np.sqrt(v) + eps), m, v


# ---- the small separable task of "it learns" --------------------------------------------------------------------------------------
TASK_CLASSES, TASK_BATCH, TASK_STEPS, TASK_LR, TASK_HELD_OUT = 4, 16, 250, 2e-3, 64
TASK_MASK_SEEDS = (1, 2, 3)
# held-out accuracy the float64 oracle reaches after TASK_STEPS steps under mask seeds 1, 2, 3 (test_dscnn_train_cpu.py asserts them;
# DESIGN.md section 30 records them), and what the device -- with another mask seed -- must reach: the lowest minus their spread
TASK_ORACLE_ACCURACY = (1.0, 0.96875, 1.0)
TASK_BAR = min(TASK_ORACLE_ACCURACY) - (max(TASK_ORACLE_ACCURACY) - min(TASK_ORACLE_ACCURACY))


def task_clips(n, seed):
    """n clips of TASK_CLASSES classes: structured_clips' noise floor with ONE class-dependent blob (its time x frequency position is the
    class) -> (clips [n,49,40] float32, labels [n] int32)."""
    rng = np.random.default_rng(seed)
    centres = [(10.0, 8.0), (10.0, 30.0), (36.0, 8.0), (36.0, 30.0)]
    tt, ff = np.meshgrid(np.arange(49.0), np.arange(40.0), indexing="ij")
    labels = (np.arange(n) % TASK_CLASSES).astype(np.int32)
    out = np.zeros((n, 49, 40), np.float64)
    for i in range(n):
        ct, cf = centres[labels[i]]
        ct, cf = ct + rng.uniform(-3, 3), cf + rng.uniform(-3, 3)
        x = rng.uniform(0.0, 60.0, (49, 40))
        x += rng.uniform(200.0, 400.0) * np.exp(-0.5 * (((tt - ct) / rng.uniform(3.0, 6.0)) ** 2 + ((ff - cf) / rng.uniform(2.0, 5.0)) ** 2))
        out[i] = np.floor(x)
    return out.astype(np.float32), labels


def task_batches():
    """The TASK_STEPS training batches (the same for the oracle and the device) and the held-out set."""
    train = [task_clips(TASK_BATCH, 1000 + s) for s in range(TASK_STEPS)]
    return train, task_clips(TASK_HELD_OUT, 99)


def task_start():
    return dscnn.synthetic_params(TASK_CLASSES, 77)


def oracle_train(mask_seed):
    """Trains task_start() for TASK_STEPS steps in float64 (weight_decay 1e-4, masks of dropout_mask_host under mask_seed) ->
    held-out accuracy of the evaluation-mode network."""
    named = tensors64(task_start())
    m = {n: np.zeros_like(v) for n, v in named.items() if trainable(n)}
    v = {n: np.zeros_like(w) for n, w in named.items() if trainable(n)}
    train, (held_x, held_y) = task_batches()
    for s, (x, y) in enumerate(train):
        r = step(named, x, y, host_masks(mask_seed, s, TASK_BATCH), weight_decay=1e-4)
        for n in m:
            if n in CONV_BIASES:
                continue                                       # gradient zero up to rounding noise: defined as zero
            named[n], m[n], v[n] = adam(named[n], r["grads"][n], m[n], v[n], s + 1, TASK_LR)
        named.update(r["moving"])
    return float((eval_logits(named, held_x).argmax(axis=1) == held_y).mean())
