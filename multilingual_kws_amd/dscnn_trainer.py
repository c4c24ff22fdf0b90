"""Training the DS-CNN baseline on the device: the tape of one optimizer step of the reference's train()
(notebooks/dscnn_comparison.py:147-195 on model_def :45-102).

Keras owns that graph in the reference; here the tape is host code over the C-ABI training operators of include/mkws.h -- the
mkws_op_* operators of csrc/mkws_train.hip (GEMMs, the depthwise and 1x1 convolutions with their training-mode BatchNorm, the
BatchNorm backward, cross-entropy, Adam) and the DS-CNN's own of csrc/mkws_dscnn_train.hip (the 10x4 stride-2 stem and its weight
gradient, counter-based dropout, the dropout + pool over rows 0..23).  PyTorch provides device memory and streams only.

Parameters, gradients and Adam moments are flat device buffers in the Keras-order blob of dscnn.manifest.  Semantics are Keras'
defaults: BatchNorm momentum 0.99 / eps 1e-3 on the statistics of all B * 500 rows (row 24 included), moving variance Bessel-corrected,
Dropout(0.2) behind the stem's ReLU and Dropout(0.4) in front of the pool, L2(weight_decay) on the nine convolution kernels (not the
dense kernel), loss from logits through log-softmax.

Conv biases: each of the nine convolutions carries a Keras bias in front of its BatchNorm.  Under batch statistics the batch mean
removes it, so its true gradient is exactly zero; here it is DEFINED as zero -- the biases never change and are not added to Z.  The
device keeps the moving mean of Z; params() exports the moving mean of Z + bias, so that dscnn.fold stays right for an imported
checkpoint with non-zero biases.

The class sits on op_tape.OpTape (operator context, flat state, layer calls, graph capture; shared with the embedding's trainer)."""
import ctypes

import numpy as np

from . import _lib, dscnn, synth
from .op_tape import ACT_NONE, ACT_RELU, BN_EPS, BN_MOMENTUM, OpTape  # noqa: F401
H, W, C, PIX = dscnn.OUT_H, dscnn.OUT_W, dscnn.CHANNELS, dscnn.OUT_H * dscnn.OUT_W
SITE_STEM, SITE_POOL = 0, 1
_GOLDEN = np.uint64(0x9E3779B97F4A7C15)


def dropout_mask_host(seed, step, site, n, rate):
    """The keep decisions (bool [n]) of mkws_op_dropout_* / mkws_op_dscnn_pool_* for elements 0..n-1, bit for bit."""
    with np.errstate(over="ignore"):
        base = synth.splitmix64(np.asarray([seed], dtype=np.uint64))
        base = synth.splitmix64(base + np.uint64(step))
        base = synth.splitmix64(base + np.uint64(site))
        h = synth.splitmix64(base + (np.arange(int(n), dtype=np.uint64) + np.uint64(1)) * _GOLDEN)
    thresh = np.uint64(int(np.float32(rate) * np.float32(16777216.0)))
    return (h >> np.uint64(40)) >= thresh


def dropout_scale(rate):
    """The float32 factor kept values are multiplied by."""
    return np.float32(1.0) / (np.float32(1.0) - np.float32(rate))


def _layers():
    """[(kind, kernel, bias, BatchNorm prefix)] of the nine convolutions in order."""
    out = [("stem", "conv2d/kernel", "conv2d/bias", "batch_normalization")]
    for b in range(dscnn.N_BLOCKS):
        out.append(("dw", dscnn._numbered("depthwise_conv2d", b) + "/depthwise_kernel", dscnn._numbered("depthwise_conv2d", b) + "/bias",
                    dscnn._numbered("batch_normalization", 2 * b + 1)))
        out.append(("pw", dscnn._numbered("conv2d", b + 1) + "/kernel", dscnn._numbered("conv2d", b + 1) + "/bias",
                    dscnn._numbered("batch_normalization", 2 * b + 2)))
    return out


LAYERS = _layers()
CONV_KERNELS = [k for _, k, _, _ in LAYERS]
CONV_BIASES = [b for _, _, b, _ in LAYERS]


class DSCNNTrainer(OpTape):
    def __init__(self, params, label_count=None, max_batch=1024, seed=0, weight_decay=1e-4, dropout=(0.2, 0.4), device=None, mode="eager", scratch=None):
        if mode not in ("eager", "hipgraph"):
            raise ValueError(f"mode {mode!r}: 'eager' or 'hipgraph'")
        self.mode = mode
        blob = np.ascontiguousarray(params, dtype=np.float32).copy()
        self.label_count = int(label_count) if label_count is not None else dscnn.label_count_of(blob)
        if blob.shape[0] != dscnn.param_count(self.label_count):
            raise ValueError(f"blob has {blob.shape[0]} floats, a DS-CNN of {self.label_count} labels needs {dscnn.param_count(self.label_count)}")
        if not np.all(np.isfinite(blob)):
            raise ValueError("parameter blob has a non-finite value")
        self.max_batch, self.seed, self.weight_decay = int(max_batch), int(seed) & 0xFFFFFFFFFFFFFFFF, float(weight_decay)
        self.rates = (float(dropout[0]), float(dropout[1]))
        if self.max_batch < 1 or not all(0.0 <= r < 1.0 for r in self.rates) or self.weight_decay < 0:
            raise ValueError("max_batch >= 1, dropout rates in [0, 1) and weight_decay >= 0 are required")
        # scratch: a caller-provided arena (float32, on this device, contiguous) for the fixed-order reductions; None allocates 4 Mi floats
        OpTape.__init__(self, device, scratch, 4 << 20)
        # the device keeps the moving mean of Z (see the module docstring); the biases themselves stay in the blob untouched
        host = dscnn.unpack(blob)
        for _, _, bias, bn in LAYERS:
            host[bn + "/moving_mean"] -= host[bias]
        # grads: conv biases and moving statistics are never written, exactly zero; d_step: optimizer steps done, Adam's index and the masks' counter
        self.params_dev = self._flat_state(blob, dscnn.manifest(self.label_count))
        self.stats = self.torch.zeros(2, dtype=self.torch.float32, device=self.device)
        self._ws, self._graphs = {}, {}
        self._last_B = None

    def _workspace(self, B):
        """The tape's buffers for batch B.  Batches that have a captured graph keep theirs; of the others only the last one is kept."""
        ws = self._ws.get(B)
        if ws is None:
            torch, dev, M, Lc = self.torch, self.device, B * PIX, self.label_count
            f = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)
            ws = dict(Z=[f(M, C) for _ in LAYERS], A=[f(M, C) for _ in LAYERS], mean=[f(C) for _ in LAYERS], var=[f(C) for _ in LAYERS],
                      g=[f(M, C), f(M, C)], pooled=f(B, C), dpooled=f(B, C), Zl=f(B, Lc), logits=f(B, Lc), rowstat=f(B, 2),
                      spec=torch.zeros((B, 49, 40), dtype=torch.float32, device=dev), labels=torch.zeros(B, dtype=torch.int32, device=dev))
            for old in [b for b in self._ws if b not in {k[0] for k in self._graphs}]:
                del self._ws[old]
            self._ws[B] = ws
        return ws

    def _prep(self, spec, labels):
        torch = self.torch
        if not torch.is_tensor(spec):
            spec = torch.from_numpy(np.array(spec, dtype=np.float32))
        spec = spec.to(self.device, dtype=torch.float32)
        if spec.dim() == 4 and spec.shape[-1] == 1:
            spec = spec[..., 0]
        if spec.dim() != 3 or tuple(spec.shape[1:]) != dscnn.SPEC_SHAPE:
            raise ValueError(f"expected [B,49,40] or [B,49,40,1], got {tuple(spec.shape)}")
        B = spec.shape[0]
        if not 1 <= B <= self.max_batch:
            raise ValueError(f"batch {B} outside [1, max_batch={self.max_batch}]")
        if not torch.is_tensor(labels):
            labels = torch.from_numpy(np.array(labels, dtype=np.int32))
        labels = labels.to(self.device, dtype=torch.int32).reshape(-1)
        if labels.shape[0] != B:
            raise ValueError(f"{labels.shape[0]} labels for {B} clips")
        return spec.contiguous(), labels.contiguous(), B

    # ---- one step -------------------------------------------------------------------------------------------------------
    def _tape(self, ws, B):
        """Forward, loss, backward and L2 on ws['spec'] / ws['labels']: fills self.grads and self.stats."""
        L, p, s, M, Lc = self.L, self._p, self._stream, B * PIX, self.label_count
        seed, d_step = ctypes.c_uint64(self.seed), p(self.d_step)
        Z, A, mean, var = ws["Z"], ws["A"], ws["mean"], ws["var"]
        # ---- forward
        _lib.check(L.mkws_op_dscnn_stem_fwd(p(ws["spec"]), self.P("conv2d/kernel"), p(Z[0]), B, s))
        self.bn_fwd(Z[0], M, C, LAYERS[0][3], ACT_RELU, mean[0], var[0], A[0])
        _lib.check(L.mkws_op_dropout_fwd(p(A[0]), p(A[0]), M * C, self.rates[0], seed, d_step, SITE_STEM, s))
        for i in range(1, len(LAYERS)):
            kind, kernel, _, prefix = LAYERS[i]
            if kind == "dw":
                self.dwconv_bn_fwd(A[i - 1], kernel, Z[i], B, H, W, C, 3, 1, 1, 1, H, W, prefix, ACT_RELU, mean[i], var[i], A[i])
            else:
                self.conv_bn_fwd(A[i - 1], kernel, Z[i], M, C, C, prefix, ACT_RELU, mean[i], var[i], A[i])
        _lib.check(L.mkws_op_dscnn_pool_fwd(p(A[-1]), B, self.rates[1], seed, d_step, SITE_POOL, p(ws["pooled"]), s))
        _lib.check(L.mkws_op_gemm(p(ws["pooled"]), self.P("dense/kernel"), p(ws["Zl"]), B, Lc, C, C, Lc, Lc, 0, 0, 0, 0, s))
        _lib.check(L.mkws_op_bias_act_fwd(p(ws["Zl"]), self.P("dense/bias"), ACT_NONE, p(ws["logits"]), B, Lc, s))
        # ---- loss and the dense layer's backward: logits <- d(mean loss) / d(logits)
        self.dense_ce_bwd(ws["pooled"], ws["Zl"], ws["logits"], ws["labels"], B, C, Lc, "dense", ws["rowstat"], self.stats, ws["dpooled"])
        # ---- backward
        g, other = ws["g"]
        _lib.check(L.mkws_op_dscnn_pool_bwd(p(ws["dpooled"]), B, self.rates[1], seed, d_step, SITE_POOL, p(g), s))
        for i in range(len(LAYERS) - 1, 0, -1):
            kind, kernel, _, prefix = LAYERS[i]
            self.bn_bwd(Z[i], mean[i], var[i], M, C, prefix, ACT_RELU, g, g)          # g: dLoss/dA[i] -> dLoss/dZ[i], in place
            if kind == "pw":
                _lib.check(L.mkws_op_gemm(p(A[i - 1]), p(g), self.G(kernel), C, C, M, C, C, C, 1, 0, 0, 0, s))
                _lib.check(L.mkws_op_gemm(p(g), self.P(kernel), p(other), M, C, C, C, C, C, 0, 1, 0, 0, s))
            else:
                _lib.check(L.mkws_op_dwconv_bwd(p(A[i - 1]), self.P(kernel), p(g), p(other), self.G(kernel), B, H, W, C, 3, 1, 1, 1, H, W, s))
            g, other = other, g
        _lib.check(L.mkws_op_dropout_bwd(p(g), p(g), M * C, self.rates[0], seed, d_step, SITE_STEM, s))
        self.bn_bwd(Z[0], mean[0], var[0], M, C, LAYERS[0][3], ACT_RELU, g, g)
        _lib.check(L.mkws_op_dscnn_stem_bwd_weight(p(ws["spec"]), p(g), self.G("conv2d/kernel"), B, s))
        # ---- L2 on the nine convolution kernels: grad += 2 * weight_decay * W
        if self.weight_decay > 0:
            for kernel in CONV_KERNELS:
                _lib.check(L.mkws_op_axpy(self.G(kernel), self.P(kernel), 2.0 * self.weight_decay, self.tensors[kernel]["count"], s))

    def _adam_inc(self, lr, beta1, beta2, eps):
        _lib.check(self.L.mkws_op_step_inc(self._p(self.d_step), self._stream))
        self._adam_dev(lr, beta1, beta2, eps)

    def forward_backward(self, spec, labels):
        """spec [B,49,40(,1)], labels [B] -> device stats [sum of row losses, #correct]; the gradients are in named_grads().  BatchNorm's
        moving statistics are updated (Keras does it in the training-mode forward pass); the step counter is not."""
        spec, labels, B = self._prep(spec, labels)
        with self.torch.cuda.device(self.device):
            self.bind()
            ws = self._workspace(B)
            ws["spec"].copy_(spec)
            ws["labels"].copy_(labels)
            self._tape(ws, B)
        self._last_B = B
        return self.stats

    def adam_step(self, lr, beta1=0.9, beta2=0.999, eps=1e-7):
        """Keras Adam over the whole blob: conv biases and moving statistics have zero gradient and zero moments and stay put."""
        with self.torch.cuda.device(self.device):
            self.bind()
            self._adam_inc(float(lr), beta1, beta2, eps)

    def step(self, spec, labels, lr):
        """forward_backward + adam_step; in mode "hipgraph" one replay of the graph recorded for (B, lr)."""
        if self.mode != "hipgraph":
            stats = self.forward_backward(spec, labels)
            self.adam_step(lr)
            return stats
        spec, labels, B = self._prep(spec, labels)
        with self.torch.cuda.device(self.device):
            key = (B, float(lr))
            graph = self._graphs.get(key)
            if graph is None:
                try:
                    graph = self._graphs[key] = self._capture(B, float(lr))
                except Exception:
                    self._graphs.pop(key, None)
                    raise
            ws = self._ws[B]
            ws["spec"].copy_(spec)
            ws["labels"].copy_(labels)
            graph.replay()
        self._last_B = B
        return self.stats

    def _capture(self, B, lr):
        """Records forward + loss + backward + Adam of one step on one stream.  The warm-up runs the step once on a side stream (first
        launches load code objects) on state that is restored afterwards; every counter lives in device memory."""
        self._graphs[(B, lr)] = None                           # (pins the workspace of B while it is created)
        ws = self._workspace(B)

        def body():
            self.bind()
            self._tape(ws, B)
            self._adam_inc(lr, 0.9, 0.999, 1e-7)
        return self.capture_step(body, (self.params_dev, self.grads, self.m, self.v, self.d_step, self.stats))[0]

    # ---- reading the state ------------------------------------------------------------------------------------------------
    def params(self):
        """The Keras-order blob, moving statistics included (the moving means as Keras holds them: of Z + bias), so that
        dscnn.DSCNN(trainer.params()) is the trained classifier."""
        blob = self.params_dev.cpu().numpy().copy()
        host = dscnn.unpack(blob)
        for _, _, bias, bn in LAYERS:
            host[bn + "/moving_mean"] += host[bias]
        return blob

    def batch_statistics(self):
        """{BatchNorm prefix: (mean of Z + bias [64], biased variance [64])} of the last forward pass."""
        if self._last_B is None:
            raise RuntimeError("batch_statistics() needs a forward pass first")
        ws, host = self._ws[self._last_B], dscnn.unpack(self.params_dev.cpu().numpy())
        return {bn: (ws["mean"][i].cpu().numpy() + host[bias], ws["var"][i].cpu().numpy()) for i, (_, _, bias, bn) in enumerate(LAYERS)}

    @property
    def step_count(self):
        return int(self.d_step.cpu()[0])

    def regularization_loss(self):
        """weight_decay * sum of the squared entries of the nine convolution kernels (what Keras adds to the reported loss)."""
        return dscnn.l2_penalty([self.view(kernel) for kernel in CONV_KERNELS], self.weight_decay)
