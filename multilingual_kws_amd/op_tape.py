"""The base of every host tape over the C-ABI training operators of include/mkws.h (`mkws_op_*`, csrc/mkws_train.hip): EmbeddingTrainer
(embedding_trainer.py), DSCNNTrainer (dscnn_trainer.py) and LogitsLayer (train_multilingual_embedding.py) derive from OpTape.

What they share lives here once: the library handle and the operator context over a scratch arena (create, bind, destroy), the flat device
state params | grads | m | v built from a blob and its manifest with one cached pointer lookup by tensor name, Keras Adam with a host or a
device step index, the warm-up / restore / capture recipe of a graphed step, and the layer calls that carry BatchNormalization's four
tensors (resolved from the layer's prefix) or the dense + softmax-cross-entropy tail.  The layer calls take every buffer from the caller: a
tape keeps its own buffer policy (a call-order pool, a per-batch workspace).

Every library call goes through the instance attribute `self.L`: embedding_trainer.TrainStepGraph swaps it for a call recorder."""
import ctypes

from . import _lib

BN_EPS, BN_MOMENTUM = 1e-3, 0.99
ACT_NONE, ACT_SWISH, ACT_RELU, ACT_SELU, ACT_SIGMOID = 0, 1, 2, 3, 4


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


class OpTape:
    _p = staticmethod(_p)

    def __init__(self, device=None, scratch=None, scratch_floats=16 << 20):
        """scratch: the caller's arena for the fixed-order reductions (mkws_train_ctx), None allocates scratch_floats floats."""
        import torch
        self.torch, self.L = torch, _lib.lib()
        self.device = _lib.indexed_device(device)
        self._stream = None
        self._views, self._ptrs, self._bn = {}, {}, {}
        # the tape's own operator context (arena + deferred-fold queue): independent of other tapes on this thread and of the thread it
        # runs on; bound at the top of every public method (bind)
        self._scratch, self._ctx = self._new_ctx(scratch, scratch_floats)

    def _arena(self, t):
        torch = self.torch
        if not (isinstance(t, torch.Tensor) and t.dtype == torch.float32 and t.device == self.device and t.dim() == 1 and t.is_contiguous() and t.numel() > 0):
            raise ValueError(f"a scratch arena is a contiguous one-dimensional float32 tensor on {self.device}")
        return t

    def _new_ctx(self, arena, floats):
        """-> (arena, operator context over it); arena None: `floats` floats are allocated."""
        arena = self._arena(arena) if arena is not None else self.torch.empty(floats, dtype=self.torch.float32, device=self.device)
        ctx = ctypes.c_void_p()
        _lib.check(self.L.mkws_train_ctx_create(_p(arena), arena.numel(), ctypes.byref(ctx)))
        return arena, ctx

    def __del__(self):
        try:
            for name in ("_ctx", "_ctx_side"):
                if getattr(self, name, None):
                    self.L.mkws_train_ctx_destroy(getattr(self, name))
                    setattr(self, name, None)
        except Exception:
            pass

    def bind(self):
        """Latches torch's current stream and makes this tape's operator context the thread's (a thread-local pointer store)."""
        self._stream = _lib.current_stream_ptr()
        _lib.check(self.L.mkws_train_ctx_bind(self._ctx))

    # ---- flat state -----------------------------------------------------------------------------------------------------
    def _flat_state(self, blob, manifest):
        """Flat device buffers in the blob's own order: returns the parameters; gradients, Adam moments and the device step index become
        self.grads / .m / .v / .d_step, the manifest self.tensors."""
        torch = self.torch
        self.tensors = {t["name"]: t for t in manifest}
        self._params = torch.from_numpy(blob).to(self.device)
        self.grads, self.m, self.v = (torch.zeros_like(self._params) for _ in range(3))
        self.d_step = torch.zeros(1, dtype=torch.int32, device=self.device)
        return self._params

    def view(self, name, buf=None):
        """Tensor `name`'s slice of a flat buffer (default: the parameters)."""
        buf = self._params if buf is None else buf
        v = self._views.get((id(buf), name))
        if v is None:
            t = self.tensors[name]
            v = self._views[(id(buf), name)] = buf[t["offset"]:t["offset"] + t["count"]]
        return v

    def P(self, name):
        """Pointer of parameter tensor `name` (the flat buffers stay put: looked up once)."""
        p = self._ptrs.get(name)
        if p is None:
            p = self._ptrs[name] = _p(self.view(name))
        return p

    def G(self, name):
        """Pointer of tensor `name`'s gradient."""
        p = self._ptrs.get(("g", name))
        if p is None:
            p = self._ptrs[("g", name)] = _p(self.view(name, self.grads))
        return p

    def _bn_ptrs(self, prefix):
        """(gamma, beta, moving mean, moving variance, dgamma, dbeta) of the BatchNormalization layer `prefix`."""
        b = self._bn.get(prefix)
        if b is None:
            b = self._bn[prefix] = tuple(self.P(prefix + leaf) for leaf in ("/gamma", "/beta", "/moving_mean", "/moving_variance")) + (
                self.G(prefix + "/gamma"), self.G(prefix + "/beta"))
        return b

    def named_grads(self):
        g = self.grads.cpu().numpy()
        return {n: g[t["offset"]:t["offset"] + t["count"]].reshape(t["shape"]) for n, t in self.tensors.items()}

    def _adam(self, lr, beta1, beta2, eps, step_t, grad_scale=1.0):
        """Keras Adam over the whole flat state on the latched stream, host step index."""
        _lib.check(self.L.mkws_op_adam(_p(self._params), _p(self.grads), _p(self.m), _p(self.v), self._params.shape[0], lr, beta1, beta2, eps, step_t, grad_scale,
                                       self._stream))

    def _adam_dev(self, lr, beta1, beta2, eps, grad_scale=1.0):
        """The same update with the step index read from self.d_step on the device (graph-replayed steps)."""
        _lib.check(self.L.mkws_op_adam_dev(_p(self._params), _p(self.grads), _p(self.m), _p(self.v), self._params.shape[0], lr, beta1, beta2, eps, _p(self.d_step),
                                           grad_scale, self._stream))

    # ---- one step as a graph ----------------------------------------------------------------------------------------------
    def capture_step(self, body, state, restore_extra=None):
        """body() once on a side stream (first launches load code objects, fill buffer pools and lazily created views) on `state` -- device
        tensors, restored afterwards; restore_extra() puts back what lives on the host -- then body() captured -> (graph, body's result)."""
        torch, dev = self.torch, self.device
        snap = [t.clone() for t in state]
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            body()
        torch.cuda.current_stream(dev).wait_stream(side)
        torch.cuda.synchronize(dev)
        for t, c in zip(state, snap):
            t.copy_(c)
        if restore_extra is not None:
            restore_extra()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = body()
        return graph, out

    # ---- layer calls: every buffer is the caller's ------------------------------------------------------------------------
    def bn_fwd(self, Z, M, C, prefix, act, mean, var, A, res=None, row_scale=None, group=1):
        """Training-mode BN + activation: batch statistics + moving-average update (Keras does it during the training-mode forward pass) +
        normalise / activate; res / row_scale [M // group]: A = row_scale * act(BN(Z)) + res in the same launch."""
        g, b, mm, mv = self._bn_ptrs(prefix)[:4]
        _lib.check(self.L.mkws_op_bn_train_fwd_res(_p(Z), M, C, g, b, BN_EPS, act, BN_MOMENTUM, mm, mv, _p(mean), _p(var), _p(A), _p(res), _p(row_scale), group,
                                                   self._stream))

    def bn_bwd(self, Z, mean, var, M, C, prefix, act, dA, src, row_scale=None, bcast=None, bscale=0.0, group=1):
        """dLoss/dA -> dLoss/dZ in dA [M,C]; writes dgamma / dbeta.  The incoming gradient is src (None: none) * row_scale[row // group]
        + bcast[row // group] * bscale, assembled inside the first launch."""
        g, b, _, _, dg, db = self._bn_ptrs(prefix)
        _lib.check(self.L.mkws_op_bn_act_bwd_ex(_p(Z), _p(mean), _p(var), g, b, BN_EPS, act, _p(dA), _p(src), _p(row_scale), _p(bcast), float(bscale), group, dg, db,
                                                M, C, self._stream))

    def conv_bn_fwd(self, X, wname, Z, M, N, K, prefix, act, mean, var, A, res=None, row_scale=None, group=1):
        """1x1 convolution + training-mode BN (+ activation / residual branch) as one operator: the GEMM's epilogue leaves the BN's chunk
        statistics whenever it can."""
        g, b, mm, mv = self._bn_ptrs(prefix)[:4]
        _lib.check(self.L.mkws_op_conv_bn_fwd(_p(X), self.P(wname), _p(Z), M, N, K, g, b, BN_EPS, act, BN_MOMENTUM, mm, mv, _p(mean), _p(var), _p(A), _p(res),
                                              _p(row_scale), group, self._stream))

    def dwconv_bn_fwd(self, X, wname, Z, B, H, W, C, k, s, pt, pl, Ho, Wo, prefix, act, mean, var, A):
        """Depthwise convolution + training-mode BN + activation: the convolution launch leaves the BN chunk statistics."""
        g, b, mm, mv = self._bn_ptrs(prefix)[:4]
        _lib.check(self.L.mkws_op_dwconv_bn_fwd(_p(X), self.P(wname), _p(Z), B, H, W, C, k, s, pt, pl, Ho, Wo, g, b, BN_EPS, act, BN_MOMENTUM, mm, mv, _p(mean),
                                                _p(var), _p(A), self._stream))

    def dense_ce_bwd(self, X, Z, logits, labels, B, K, N, prefix, rowstat, stats, dX):
        """The tail of a classifier, logits = X [B,K] @ kernel + bias with pre-activation Z: mean sparse cross-entropy from logits (stats =
        [sum of row losses, #correct]) leaves d(mean loss)/d(logits) in `logits`; dbias = its column sums (the identity activation's
        backward leaves it untouched), dkernel = X^T d, dX = d kernel^T."""
        L, s, d = self.L, self._stream, _p(logits)
        _lib.check(L.mkws_op_softmax_ce(d, _p(labels), B, N, _p(rowstat), _p(stats), s))
        _lib.check(L.mkws_op_bias_act_bwd(_p(Z), self.P(prefix + "/bias"), ACT_NONE, d, self.G(prefix + "/bias"), B, N, s))
        _lib.check(L.mkws_op_gemm(_p(X), d, self.G(prefix + "/kernel"), K, N, B, K, N, N, 1, 0, 0, 0, s))
        _lib.check(L.mkws_op_gemm(d, self.P(prefix + "/kernel"), _p(dX), B, K, N, N, N, K, 0, 1, 0, 0, s))
