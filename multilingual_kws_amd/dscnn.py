"""The DS-CNN baseline the reference measures the few-shot models against (notebooks/dscnn_comparison.py:45-102 model_def): import,
inference on the device (mkws_dscnn_* of include/mkws.h, one launch per forward), and its specification on the host.

Parameters are a flat float32 blob in Keras variable order and layout, BatchNorm tensors included (manifest()).  The device sees folded
weights only: fold() is the specification of what mkws_dscnn_create does with the blob, dscnn_host the specification of the forward
pass -- float64 NumPy on the float32 folded weights, written from the layer list in include/mkws.h.  Training is dscnn_trainer.py
(DESIGN.md section 30)."""
import contextlib
import ctypes
import json
import os
import re

import numpy as np

from . import _lib

SPEC_SHAPE = (49, 40)
OUT_H, OUT_W, CHANNELS = 25, 20, 64
POOL_ROWS = 24                    # int(49 / 2): AveragePooling2D((24, 20)), valid -- row 24 is computed and not pooled
BN_EPS = 1e-3
MIN_LABELS, MAX_LABELS = 2, 64
N_BLOCKS = 4
TRUNK_PARAMS = 24128
FORMAT = "mkws-dscnn-v1"


def param_count(label_count):
    n = int(_lib.lib().mkws_dscnn_param_count(int(label_count)))
    if n == 0:
        raise ValueError(f"label_count {label_count} outside [{MIN_LABELS}, {MAX_LABELS}]")
    return n


def manifest(label_count):
    """[{name, shape, offset, count}] straight from the C library (host-only call, no GPU needed)."""
    L = _lib.lib()
    n = _lib.check(L.mkws_dscnn_weight_manifest(int(label_count), None, 0))
    buf = ctypes.create_string_buffer(n + 1)
    _lib.check(L.mkws_dscnn_weight_manifest(int(label_count), buf, n + 1))
    return json.loads(buf.value.decode("utf-8"))["tensors"]


def label_count_of(params):
    n = int(np.asarray(params).shape[0])
    L, rest = divmod(n - TRUNK_PARAMS, CHANNELS + 1)
    if rest or not MIN_LABELS <= L <= MAX_LABELS:
        raise ValueError(f"{n} parameters are no DS-CNN of {MIN_LABELS}..{MAX_LABELS} labels ({TRUNK_PARAMS} + 65 * label_count)")
    return L


def unpack(params):
    """blob -> {Keras variable name: float32 view of its shape}."""
    params = np.asarray(params, dtype=np.float32)
    return {t["name"]: params[t["offset"]:t["offset"] + t["count"]].reshape(t["shape"]) for t in manifest(label_count_of(params))}


def _numbered(kind, i):
    return kind if i == 0 else f"{kind}_{i}"


WEIGHT_DECAY = 1e-4               # the reference's model_def: L2(1e-4) on every convolution kernel


def conv_kernel_names():
    """The nine convolution kernels in layer order (stem, then depthwise and pointwise of every block): what the L2 penalty covers."""
    names = ["conv2d/kernel"]
    for b in range(N_BLOCKS):
        names += [_numbered("depthwise_conv2d", b) + "/depthwise_kernel", _numbered("conv2d", b + 1) + "/kernel"]
    return names


def l2_penalty(kernels, weight_decay):
    """weight_decay * the sum of the squared entries of `kernels` (torch tensors on any device), each kernel summed in float64: the
    one formula behind DSCNNTrainer.regularization_loss and DSCNN.evaluate."""
    total = 0.0
    for w in kernels:
        total = total + w.double().square().sum()
    return float(weight_decay) * float(total)


_KINDS = {"conv2d": 1 + N_BLOCKS, "depthwise_conv2d": N_BLOCKS, "batch_normalization": 1 + 2 * N_BLOCKS, "dense": 1}
_LEAVES = {"conv2d": ("kernel", "bias"), "depthwise_conv2d": ("depthwise_kernel", "bias"),
           "batch_normalization": ("gamma", "beta", "moving_mean", "moving_variance"), "dense": ("kernel", "bias")}
_NAME = re.compile(r"^(conv2d|depthwise_conv2d|batch_normalization|dense)(?:_(\d+))?/([a-z_]+)$")


def from_named_tensors(named):
    """{Keras variable name: ndarray}, as checkpoint_import.load_h5 / load_savedmodel name them, -> blob.  Keras numbers auto-named
    layers from a per-session counter, so the layers of each kind are ordered by their numeric suffix (none = 0), whatever it starts at.
    ValueError for a set whose kinds, counts or shapes do not make this network."""
    layers = {k: {} for k in _KINDS}
    for name, value in named.items():
        m = _NAME.match(name.split(":")[0])
        if not m:
            raise ValueError(f"'{name}' is no variable of a DS-CNN (layers are conv2d, depthwise_conv2d, batch_normalization, dense)")
        layers[m.group(1)].setdefault(int(m.group(2) or 0), {})[m.group(3)] = value
    for kind, want in _KINDS.items():
        if len(layers[kind]) != want:
            raise ValueError(f"{len(layers[kind])} {kind} layers, a DS-CNN has {want}")
    dense = layers["dense"][min(layers["dense"])]
    if "kernel" not in dense or np.ndim(dense["kernel"]) != 2:
        raise ValueError("dense layer without a [64, label_count] kernel")
    label_count = int(np.shape(dense["kernel"])[1])
    if not MIN_LABELS <= label_count <= MAX_LABELS:
        raise ValueError(f"label_count {label_count} outside [{MIN_LABELS}, {MAX_LABELS}]")
    order = {kind: sorted(layers[kind]) for kind in _KINDS}
    blob = np.zeros(param_count(label_count), dtype=np.float32)
    for t in manifest(label_count):
        m = _NAME.match(t["name"])
        have = layers[m.group(1)][order[m.group(1)][int(m.group(2) or 0)]]
        if m.group(3) not in have:
            raise ValueError(f"{t['name']}: the layer holds {sorted(have)}, no '{m.group(3)}'")
        v = np.asarray(have[m.group(3)], dtype=np.float32)
        if list(v.shape) != list(t["shape"]):
            raise ValueError(f"{t['name']}: shape {list(v.shape)}, a DS-CNN needs {t['shape']}")
        blob[t["offset"]:t["offset"] + t["count"]] = v.reshape(-1)
    for kind in _KINDS:
        for i in order[kind]:
            extra = set(layers[kind][i]) - set(_LEAVES[kind])
            if extra:
                raise ValueError(f"{kind} layer {i} holds unexpected variables {sorted(extra)}")
    return blob


def _fold_one(w, bias, gamma, beta, mean, var):
    scale = gamma.astype(np.float64) / np.sqrt(var.astype(np.float64) + np.float64(np.float32(BN_EPS)))
    return (w.astype(np.float64) * scale).astype(np.float32), ((bias.astype(np.float64) - mean.astype(np.float64)) * scale + beta.astype(np.float64)).astype(np.float32)


def fold(params):
    """What mkws_dscnn_create does: every BatchNorm folded into the convolution before it, in float64, rounded once to float32.
    -> dict(stem_w [40,64], stem_b, dw_w [4][9,64], dw_b, pw_w [4][64,64], pw_b, dense_w [64,L], dense_b)."""
    t = unpack(params)
    bn = lambda i: [t[f"{_numbered('batch_normalization', i)}/{leaf}"] for leaf in ("gamma", "beta", "moving_mean", "moving_variance")]
    out = dict(dw_w=[], dw_b=[], pw_w=[], pw_b=[])
    out["stem_w"], out["stem_b"] = _fold_one(t["conv2d/kernel"].reshape(40, CHANNELS), t["conv2d/bias"], *bn(0))
    for b in range(N_BLOCKS):
        w, bias = _fold_one(t[_numbered("depthwise_conv2d", b) + "/depthwise_kernel"].reshape(9, CHANNELS), t[_numbered("depthwise_conv2d", b) + "/bias"], *bn(2 * b + 1))
        out["dw_w"].append(w), out["dw_b"].append(bias)
        w, bias = _fold_one(t[_numbered("conv2d", b + 1) + "/kernel"].reshape(CHANNELS, CHANNELS), t[_numbered("conv2d", b + 1) + "/bias"], *bn(2 * b + 2))
        out["pw_w"].append(w), out["pw_b"].append(bias)
    out["dense_w"], out["dense_b"] = t["dense/kernel"], t["dense/bias"]
    return out


def _stem_patches(spec):
    """[B,49,40] float64 -> [B,25,20,40]: the 10x4 stride-2 windows under TensorFlow's SAME padding (top 4, bottom 5, left 1, right 1)."""
    B = spec.shape[0]
    padded = np.zeros((B, 49 + 9, 40 + 2), np.float64)
    padded[:, 4:53, 1:41] = spec
    cols = [padded[:, ky:ky + 49:2, kx:kx + 39:2] for ky in range(10) for kx in range(4)]
    return np.stack(cols, axis=-1)


def _depthwise(x, w9):
    """[B,25,20,64] float64, [9,64] -> 3x3 SAME depthwise convolution (taps in (ky, kx) order)."""
    padded = np.zeros((x.shape[0], OUT_H + 2, OUT_W + 2, CHANNELS), np.float64)
    padded[:, 1:-1, 1:-1] = x
    y = np.zeros_like(x)
    for ky in range(3):
        for kx in range(3):
            y += padded[:, ky:ky + OUT_H, kx:kx + OUT_W] * w9[3 * ky + kx]
    return y


def _forward_stages(spec, f, hook=None):
    """The layer list, float64.  `f` is fold()'s dict (or, for calibration, any dict of that shape); hook(index, pre_activation) may
    replace a convolution's output before its ReLU."""
    spec = np.asarray(spec, dtype=np.float64)
    if spec.ndim == 4 and spec.shape[-1] == 1:
        spec = spec[..., 0]
    if spec.ndim != 3 or tuple(spec.shape[1:]) != SPEC_SHAPE:
        raise ValueError(f"expected [B,49,40] or [B,49,40,1], got {tuple(spec.shape)}")
    hook = hook or (lambda i, y: y)
    stages = []
    x = np.maximum(hook(0, _stem_patches(spec) @ f["stem_w"].astype(np.float64) + f["stem_b"].astype(np.float64)), 0.0)
    stages.append(x)
    for b in range(N_BLOCKS):
        x = np.maximum(hook(2 * b + 1, _depthwise(x, f["dw_w"][b].astype(np.float64)) + f["dw_b"][b].astype(np.float64)), 0.0)
        x = np.maximum(hook(2 * b + 2, x @ f["pw_w"][b].astype(np.float64) + f["pw_b"][b].astype(np.float64)), 0.0)
        stages.append(x)
    pooled = x[:, :POOL_ROWS].mean(axis=(1, 2))
    stages.append(pooled)
    logits = pooled @ f["dense_w"].astype(np.float64) + f["dense_b"].astype(np.float64)
    return stages, logits


def softmax_host(logits):
    e = np.exp(logits - logits.max(axis=1, keepdims=True))
    return e / e.sum(axis=1, keepdims=True)


def dscnn_host(spec, params, stage=None):
    """The specification of the device forward: float64 NumPy on the float32 folded weights.  stage None -> logits [B,L]; 0..4 -> the
    stem / block output [B,25,20,64] after its last ReLU; 5 -> the pooled [B,64]; "all" -> ([stage 0..5], logits)."""
    stages, logits = _forward_stages(spec, fold(params))
    if stage is None:
        return logits
    return (stages, logits) if stage == "all" else stages[int(stage)]


def structured_clips(n, seed):
    """[n,49,40] float32 integer-valued test spectrograms: a few Gaussian blobs in time x frequency (random centres, widths, heights of
    100..400) over uniform 0..60 noise, floored.  Uniform noise alone is useless for this network: after the average pool every clip's
    features nearly coincide."""
    rng = np.random.default_rng(seed)
    tt, ff = np.meshgrid(np.arange(49.0), np.arange(40.0), indexing="ij")
    out = np.zeros((n, 49, 40), np.float64)
    for i in range(n):
        x = rng.uniform(0.0, 60.0, (49, 40))
        for _ in range(int(rng.integers(2, 6))):
            ct, cf = rng.uniform(0, 49), rng.uniform(0, 40)
            st, sf = rng.uniform(2.0, 10.0), rng.uniform(1.5, 8.0)
            x += rng.uniform(100.0, 400.0) * np.exp(-0.5 * (((tt - ct) / st) ** 2 + ((ff - cf) / sf) ** 2))
        out[i] = np.floor(x)
    return out.astype(np.float32)


def _he_normal(rng, shape, fan_in):
    return (rng.standard_normal(shape) * np.sqrt(2.0 / fan_in)).astype(np.float32)


def synthetic_params(label_count, seed=1234, calibration_clips=24):
    """Seeded random parameters: He-normal kernels, non-trivial BatchNorm scale and offset, BatchNorm moving statistics calibrated layer
    by layer on structured_clips(calibration_clips, seed + 1) so that every ReLU stays data-dependent, and a dense bias that centres
    the logits on those clips."""
    rng = np.random.default_rng(seed)
    blob = np.zeros(param_count(label_count), dtype=np.float32)
    t = unpack(blob)
    for name, v in t.items():
        leaf = name.split("/")[1]
        if leaf == "depthwise_kernel":
            v[...] = _he_normal(rng, v.shape, 9)
        elif leaf == "kernel" and v.ndim == 4:
            v[...] = _he_normal(rng, v.shape, v.shape[0] * v.shape[1] * v.shape[2])
        elif leaf == "kernel":
            v[...] = _he_normal(rng, v.shape, v.shape[0])
        elif leaf == "bias":
            v[...] = 0.02 * rng.standard_normal(v.shape)
        elif leaf == "gamma":
            v[...] = rng.uniform(0.5, 1.5, v.shape)
        elif leaf == "beta":
            v[...] = 0.1 * rng.standard_normal(v.shape)
        elif leaf == "moving_variance":
            v[...] = 1.0
    # calibration: run the unfolded layers (scale 1, bias as drawn), set each BatchNorm's statistics from what reaches it, apply it
    raw = dict(stem_w=t["conv2d/kernel"].reshape(40, CHANNELS), stem_b=t["conv2d/bias"],
               dw_w=[t[_numbered("depthwise_conv2d", b) + "/depthwise_kernel"].reshape(9, CHANNELS) for b in range(N_BLOCKS)],
               dw_b=[t[_numbered("depthwise_conv2d", b) + "/bias"] for b in range(N_BLOCKS)],
               pw_w=[t[_numbered("conv2d", b + 1) + "/kernel"].reshape(CHANNELS, CHANNELS) for b in range(N_BLOCKS)],
               pw_b=[t[_numbered("conv2d", b + 1) + "/bias"] for b in range(N_BLOCKS)],
               dense_w=t["dense/kernel"], dense_b=np.zeros(label_count, np.float32))

    def calibrate(i, y):
        p = _numbered("batch_normalization", i)
        mean, var = y.mean(axis=(0, 1, 2)), y.var(axis=(0, 1, 2))
        t[p + "/moving_mean"][...] = mean
        t[p + "/moving_variance"][...] = np.maximum(var, 1e-6)
        m32, v32 = t[p + "/moving_mean"].astype(np.float64), t[p + "/moving_variance"].astype(np.float64)
        return (y - m32) / np.sqrt(v32 + np.float64(np.float32(BN_EPS))) * t[p + "/gamma"].astype(np.float64) + t[p + "/beta"].astype(np.float64)

    _, logits = _forward_stages(structured_clips(calibration_clips, seed + 1), raw, hook=calibrate)
    t["dense/bias"][...] = -logits.mean(axis=0)
    return blob


def glorot_params(label_count, seed=None):
    """Keras' default initialisation of model_def: Glorot-uniform kernels, zero biases, BatchNorm ones and zeros."""
    rng = np.random.default_rng(seed)
    blob = np.zeros(param_count(label_count), dtype=np.float32)
    for name, v in unpack(blob).items():
        leaf = name.split("/")[1]
        if leaf in ("kernel", "depthwise_kernel"):
            field = int(np.prod(v.shape[:-2]))
            lim = np.sqrt(6.0 / (field * v.shape[-2] + field * v.shape[-1]))
            v[...] = rng.uniform(-lim, lim, v.shape)
        elif leaf in ("gamma", "moving_variance"):
            v[...] = 1.0
    return blob


def save(path, params):
    """Writes <path>/weights.bin (float32 LE) + <path>/manifest.json."""
    params = np.ascontiguousarray(params, dtype="<f4")
    label_count = label_count_of(params)
    os.makedirs(path, exist_ok=True)
    params.tofile(os.path.join(path, "weights.bin"))
    with open(os.path.join(path, "manifest.json"), "w") as f:
        json.dump({"format": FORMAT, "dtype": "float32", "label_count": label_count, "tensors": manifest(label_count)}, f)


def load(path):
    """Reads a container written by save(); validates it against the library's manifest."""
    with open(os.path.join(path, "manifest.json")) as f:
        man = json.load(f)
    if man.get("format") != FORMAT or man.get("tensors") != manifest(man.get("label_count", 0)):
        raise ValueError(f"{path}: manifest does not match this build's DS-CNN")
    params = np.fromfile(os.path.join(path, "weights.bin"), dtype="<f4")
    if params.shape[0] != param_count(man["label_count"]):
        raise ValueError(f"{path}: weights.bin has {params.shape[0]} floats, expected {param_count(man['label_count'])}")
    return params


def load_keras(path):
    """An `.h5` file (model.save / save_weights) or a SavedModel directory of the reference's model_def -> blob.  Variables of other
    objects in a SavedModel (optimizer slots, counters) are left aside; the network's own must make a DS-CNN (from_named_tensors)."""
    from . import checkpoint_import
    if os.path.isdir(path):
        info = checkpoint_import.load_savedmodel(path)
        named = {name: info["reader"].tensor(key) for name, key in info["named"].items() if _NAME.match(name)}
    else:
        named = checkpoint_import.load_h5(path)["named"]
    return from_named_tensors(named)


class DSCNN:
    """The DS-CNN on the device.  `params`: the blob (manifest order); label_count may be left out (it follows from the blob's size)."""

    def __init__(self, params, label_count=None, max_batch=1024, device=None):
        import torch
        self.L = _lib.lib()
        params = np.ascontiguousarray(params, dtype=np.float32)
        self.label_count = int(label_count) if label_count is not None else label_count_of(params)
        self.device = torch.device(device if device is not None else f"cuda:{torch.cuda.current_device()}" if torch.cuda.is_available() else "cuda:0")
        h = ctypes.c_void_p()
        # (without a device the library still checks the blob first, then says MKWS_ERR_NO_DEVICE)
        with torch.cuda.device(self.device) if torch.cuda.is_available() else contextlib.nullcontext():
            _lib.check(self.L.mkws_dscnn_create(params.ctypes.data, params.shape[0], self.label_count, int(max_batch), ctypes.byref(h)))
        self.h = h
        self.max_batch = int(max_batch)
        self.params = params
        self.grid = int(self.L.mkws_dscnn_grid(self.h))

    @classmethod
    def from_keras(cls, path, max_batch=1024, device=None):
        """An `.h5` file (model.save / save_weights) or a SavedModel directory of the reference's model_def."""
        return cls(load_keras(path), max_batch=max_batch, device=device)

    @classmethod
    def load(cls, path, max_batch=1024, device=None):
        return cls(load(path), max_batch=max_batch, device=device)

    def save(self, path):
        save(path, self.params)

    def close(self):
        if getattr(self, "h", None):
            self.L.mkws_dscnn_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _prep(self, spec):
        import torch
        if not torch.is_tensor(spec):
            spec = torch.from_numpy(np.array(spec, dtype=np.float32))         # (a copy: a read-only array must not be handed to torch)
        spec = spec.to(self.device, dtype=torch.float32)
        if spec.dim() == 4 and spec.shape[-1] == 1:
            spec = spec[..., 0]
        if spec.dim() != 3 or tuple(spec.shape[1:]) != SPEC_SHAPE:
            raise ValueError(f"expected [B,49,40] or [B,49,40,1], got {tuple(spec.shape)}")
        return spec.contiguous()

    def _run(self, spec, want_logits):
        """One launch on the current stream: (probs, logits or None), CUDA [B, label_count].  B > max_batch is refused by the library."""
        import torch
        spec = self._prep(spec)
        B = spec.shape[0]
        probs = torch.empty((B, self.label_count), dtype=torch.float32, device=self.device)
        logits = torch.empty((B, self.label_count), dtype=torch.float32, device=self.device) if want_logits else None
        with torch.cuda.device(self.device):
            _lib.check(self.L.mkws_dscnn_forward(self.h, ctypes.c_void_p(spec.data_ptr()), B, ctypes.c_void_p(probs.data_ptr()),
                                                 ctypes.c_void_p(logits.data_ptr()) if want_logits else None, _lib.current_stream_ptr()))
        return probs, logits

    def forward(self, spec):
        """spec [B,49,40(,1)] -> CUDA softmax probabilities [B, label_count]."""
        return self._run(spec, False)[0]

    def logits(self, spec):
        return self._run(spec, True)[1]

    def tap(self, spec, stage):
        """The same launch with one store added: stage 0 = stem, 1..4 = the blocks -> CUDA [B,25,20,64]; 5 -> the pooled [B,64]."""
        import torch
        spec = self._prep(spec)
        B, stage = spec.shape[0], int(stage)
        out = torch.empty((B, CHANNELS) if stage == 5 else (B, OUT_H, OUT_W, CHANNELS), dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(self.L.mkws_dscnn_tap(self.h, ctypes.c_void_p(spec.data_ptr()), B, stage, ctypes.c_void_p(out.data_ptr()), _lib.current_stream_ptr()))
        return out

    def predict(self, x, **_):
        """Keras' model.predict: [B,49,40] or [B,49,40,1] -> NumPy probabilities [B, label_count], in batches of max_batch, so that the model
        goes unchanged into transfer_learning.evaluate_files_multiclass / evaluate_fast_multiclass."""
        x = np.asarray(x, dtype=np.float32)
        if x.ndim == 4 and x.shape[-1] == 1:
            x = x[..., 0]
        if x.ndim != 3 or tuple(x.shape[1:]) != SPEC_SHAPE:
            raise ValueError(f"expected [B,49,40] or [B,49,40,1], got {tuple(x.shape)}")
        out = [self.forward(x[s:s + self.max_batch]).cpu().numpy() for s in range(0, x.shape[0], self.max_batch)]
        return np.concatenate(out) if out else np.zeros((0, self.label_count), np.float32)

    def predict_device(self, spec):
        """CUDA [N,49,40(,1)] -> CUDA probabilities [N, label_count], in launches of max_batch."""
        import torch
        outs = [self.forward(spec[s:s + self.max_batch]) for s in range(0, spec.shape[0], self.max_batch)]
        return torch.cat(outs) if outs else torch.empty((0, self.label_count), dtype=torch.float32, device=self.device)

    def regularization_loss(self, weight_decay=WEIGHT_DECAY):
        """What Keras adds to the loss evaluate reports: the L2 penalty of the nine convolution kernels (l2_penalty)."""
        import torch
        host = unpack(self.params)
        return l2_penalty([torch.from_numpy(np.ascontiguousarray(host[name])) for name in conv_kernel_names()], weight_decay)

    def score(self, x, y=None, batch_size=32):
        """The point scores over a ClipDataset or an array [N,49,40(,1)] with labels y: scoring.Scorer.result(), tallied on the device
        (the loss without the L2 penalty)."""
        from . import scoring
        return scoring.score_model(self.predict_device, self.device, self.label_count, 0, x, y, batch_size)

    def evaluate(self, x, y=None, batch_size=32, verbose=0, return_dict=False, weight_decay=WEIGHT_DECAY):
        """Keras' model.evaluate for the reference's compile (sparse categorical cross-entropy, SparseCategoricalAccuracy):
        [loss, sparse_categorical_accuracy] or the dict; the loss includes the L2 penalty, as Keras' does."""
        from . import scoring
        return scoring.keras_metrics(self.score(x, y, batch_size), ("loss", "sparse_categorical_accuracy"), return_dict,
                                     extra_loss=self.regularization_loss(weight_decay))
