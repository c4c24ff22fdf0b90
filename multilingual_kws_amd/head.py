"""Device few-shot head handle: host wrapper over mkws_head_* (include/mkws.h).

Dense(18,tanh) -> Dense(3,softmax) + sparse CE + Keras Adam on the frozen embedding
(multilingual_kws/embedding/transfer_learning.py:47-59).
"""
import ctypes

import numpy as np

from . import _lib


def glorot_uniform_params(in_dim=1024, hidden=18, classes=3, seed=None):
    """Keras Dense defaults: kernel glorot_uniform, bias zeros.  Flat layout W1|b1|W2|b2."""
    rng = np.random.default_rng(seed)
    l1 = np.sqrt(6.0 / (in_dim + hidden))
    l2 = np.sqrt(6.0 / (hidden + classes))
    W1 = rng.uniform(-l1, l1, (in_dim, hidden))
    W2 = rng.uniform(-l2, l2, (hidden, classes))
    return np.concatenate([W1.ravel(), np.zeros(hidden), W2.ravel(), np.zeros(classes)]).astype(np.float32)


class Head:
    def __init__(self, in_dim=1024, hidden=18, classes=3, max_batch=1024, params=None, seed=None, device=None):
        import torch
        self.L = _lib.lib()
        self.in_dim, self.hidden, self.classes = in_dim, hidden, classes
        self.device = _lib.indexed_device(device)
        h = ctypes.c_void_p()
        with torch.cuda.device(self.device):
            _lib.check(self.L.mkws_head_create(in_dim, hidden, classes, int(max_batch), ctypes.byref(h)))
        self.h = h
        self.generation = _lib.next_generation()
        self.max_batch = int(max_batch)
        self.nparams = _lib.check(self.L.mkws_head_param_count(self.h))
        self.step_t = 0
        self._views = {}
        self._stats = torch.zeros(2, dtype=torch.float32, device=self.device)
        self.set_params(params if params is not None else glorot_uniform_params(in_dim, hidden, classes, seed))

    def close(self):
        if getattr(self, "h", None):
            _lib.forget_graphs(self)
            self.L.mkws_head_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_params(self, p):
        import torch
        p = np.ascontiguousarray(p, dtype=np.float32)
        with torch.cuda.device(self.device):
            _lib.check(self.L.mkws_head_set_params(self.h, p.ctypes.data, p.shape[0], _lib.current_stream_ptr()))
        self.step_t = 0

    def get_params(self):
        import torch
        p = np.zeros(self.nparams, dtype=np.float32)
        with torch.cuda.device(self.device):
            _lib.check(self.L.mkws_head_get_params(self.h, p.ctypes.data, self.nparams, _lib.current_stream_ptr()))
        return p

    def grad_view(self, with_stats=False):
        """The flat gradient buffer as a torch tensor aliasing the handle's device memory (for RCCL).
        with_stats: the all-reduce payload [P gradients | sum of row losses | #correct] (mkws_head_grad_count)."""
        n = _lib.check(self.L.mkws_head_grad_count(self.h)) if with_stats else self.nparams
        return self._alias(self.L.mkws_head_grads(self.h), n)

    def param_view(self):
        return self._alias(self.L.mkws_head_params(self.h), self.nparams)

    def state_view(self):
        """params | grads | Adam m | Adam v as ONE flat tensor aliasing the handle (snapshot / restore of the whole optimizer state)."""
        return self._alias(self.L.mkws_head_params(self.h), _lib.check(self.L.mkws_head_state_floats(self.h)))

    def _alias(self, ptr, n):
        import torch
        key = (int(ptr), int(n))
        t = self._views.get(key)
        if t is None:
            class _Holder:   # __cuda_array_interface__ producer over raw device memory
                pass
            hld = _Holder()
            hld.__cuda_array_interface__ = {"shape": (int(n),), "typestr": "<f4", "data": (int(ptr), False), "version": 2}
            t = self._views[key] = torch.as_tensor(hld, device=self.device)
        return t

    def forward(self, emb):
        """emb CUDA [B,in] -> probs CUDA [B,classes]."""
        import torch
        B = check_forward(self.in_dim, self.device, emb)
        emb = emb.contiguous()
        probs = torch.empty((B, self.classes), dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(self.L.mkws_head_forward(self.h, ctypes.c_void_p(emb.data_ptr()), B, ctypes.c_void_p(probs.data_ptr()),
                                                _lib.current_stream_ptr()))
        return probs

    @staticmethod
    def forward_many(heads, emb):
        """N heads of equal dimensions over the same embeddings in one launch: emb CUDA [B,in] -> CUDA [N,B,classes]
        (multi-keyword serving on a shared embedding pass)."""
        import torch
        heads = list(heads)
        _, B = check_forward_many(heads, emb)
        emb = emb.contiguous()
        h0 = heads[0]
        probs = torch.empty((len(heads), B, h0.classes), dtype=torch.float32, device=h0.device)
        table = (ctypes.c_void_p * len(heads))(*[h.h.value for h in heads])
        with torch.cuda.device(h0.device):
            _lib.check(h0.L.mkws_heads_forward(table, len(heads), ctypes.c_void_p(emb.data_ptr()), B,
                                               ctypes.c_void_p(probs.data_ptr()), _lib.current_stream_ptr()))
        return probs

    def loss_grad(self, emb, labels):
        """Fills the grad buffer with d(mean CE over these rows)/d(params); returns a CUDA tensor
        [2] = {sum of row losses, number correct} (asynchronous; .tolist() syncs)."""
        import torch
        B = check_loss_grad(self.in_dim, self.device, emb, labels)
        emb = emb.contiguous()
        labels = labels.to(torch.int32).contiguous()
        with torch.cuda.device(self.device):
            _lib.check(self.L.mkws_head_loss_grad(self.h, ctypes.c_void_p(emb.data_ptr()), ctypes.c_void_p(labels.data_ptr()),
                                                  B, ctypes.c_void_p(self._stats.data_ptr()), _lib.current_stream_ptr()))
        return self._stats

    def input_grad(self, B):
        """After loss_grad on B rows: d(mean loss)/d(embedding rows), CUDA [B, in] (backprop_into_embedding)."""
        import torch
        dx = torch.empty((B, self.in_dim), dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(self.L.mkws_head_input_grad(self.h, ctypes.c_void_p(dx.data_ptr()), B, _lib.current_stream_ptr()))
        return dx

    def reset_optimizer(self):
        """A fresh Adam (zero moments, t = 0) on the current parameters -- what re-compiling the Keras model does."""
        self.set_params(self.get_params())

    def adam_step_dev(self, lr, d_step, beta1=0.9, beta2=0.999, eps=1e-7, grad_scale=1.0):
        """Adam with the step index read from the int32 device tensor d_step (graph-replayed steps: embedding_trainer.TrainStepGraph)."""
        import torch
        check_adam_step_dev(self.device, d_step)
        with torch.cuda.device(self.device):
            _lib.check(self.L.mkws_head_adam_step_dev(self.h, lr, beta1, beta2, eps, ctypes.c_void_p(d_step.data_ptr()), grad_scale, _lib.current_stream_ptr()))

    def adam_step(self, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-7, grad_scale=1.0):
        import torch
        self.step_t += 1
        with torch.cuda.device(self.device):
            _lib.check(self.L.mkws_head_adam_step(self.h, lr, beta1, beta2, eps, self.step_t, grad_scale, _lib.current_stream_ptr()))


def _check_emb(who, in_dim, device, emb):
    """emb as the single-head kernels read it once the wrapper has made it contiguous: a float32 tensor [B, in_dim] on `device` (any
    strides).  -> B."""
    import torch
    if not torch.is_tensor(emb) or emb.dim() != 2 or emb.shape[1] != in_dim or emb.dtype != torch.float32 or emb.device != device:
        got = f"{emb.dtype} {tuple(emb.shape)} on {emb.device}" if torch.is_tensor(emb) else type(emb).__name__
        raise ValueError(f"{who}: emb must be a float32 tensor [B, {in_dim}] on {device}, got {got}")
    return int(emb.shape[0])


def check_forward(in_dim, device, emb, who="Head.forward"):
    """What Head.forward refuses, decided before any device call: emb a float32 tensor [B, in_dim] on `device` (a strided view is made
    contiguous by the wrapper).  -> B.  ValueError otherwise."""
    return _check_emb(who, in_dim, device, emb)


def check_forward_many(heads, emb):
    """What Head.forward_many refuses, decided before any device call: `heads` a non-empty list of open heads (objects with in_dim,
    hidden, classes, device and a handle h) of equal dimensions on one device, emb as check_forward for them.  -> (N, B).  ValueError
    otherwise."""
    if len(heads) == 0:
        raise ValueError("Head.forward_many: heads is empty")
    if any(getattr(hd, "h", None) is None for hd in heads):
        raise ValueError("Head.forward_many: a head in heads is closed")
    h0 = heads[0]
    for k, hd in enumerate(heads):
        if (hd.in_dim, hd.hidden, hd.classes) != (h0.in_dim, h0.hidden, h0.classes):
            # (the library refuses this too, and callers caught its error before the wrapper looked: both at once)
            raise _lib.MkwsValueError(f"Head.forward_many: heads[{k}] is {hd.in_dim} x {hd.hidden} x {hd.classes}, heads[0] {h0.in_dim} x {h0.hidden} x "
                                      f"{h0.classes}: the heads must have equal dimensions")
        if hd.device != h0.device:
            raise ValueError(f"Head.forward_many: heads[{k}] lives on {hd.device}, heads[0] on {h0.device}")
    return len(heads), _check_emb("Head.forward_many", h0.in_dim, h0.device, emb)


def _check_labels(who, device, labels, B):
    """labels as the loss kernels read them once the wrapper has converted them to contiguous int32: an integer tensor [B] on `device`."""
    import torch
    if not torch.is_tensor(labels) or labels.dim() != 1 or labels.dtype not in (torch.int32, torch.int64, torch.int16, torch.int8, torch.uint8) or \
            labels.device != device:
        got = f"{labels.dtype} {tuple(labels.shape)} on {labels.device}" if torch.is_tensor(labels) else type(labels).__name__
        raise ValueError(f"{who}: labels must be an integer vector [B] on {device}, got {got}")
    if int(labels.shape[0]) != B:
        raise ValueError(f"{who}: {int(labels.shape[0])} labels for the {B} rows of emb")


def check_loss_grad(in_dim, device, emb, labels, who="Head.loss_grad"):
    """What Head.loss_grad refuses, decided before any device call: emb as check_forward; labels an integer tensor [B] on `device` (the
    wrapper converts it to contiguous int32 there), one label per row of emb.  -> B.  ValueError otherwise."""
    B = _check_emb(who, in_dim, device, emb)
    _check_labels(who, device, labels, B)
    return B


def check_adam_step_dev(device, d_step):
    """What Head.adam_step_dev refuses, decided before any device call: d_step an int32 tensor of one element on `device` (the kernel
    reads the step index through it).  ValueError otherwise."""
    import torch
    if not torch.is_tensor(d_step) or d_step.dtype != torch.int32 or d_step.numel() != 1 or d_step.device != device:
        got = f"{d_step.dtype} {tuple(d_step.shape)} on {d_step.device}" if torch.is_tensor(d_step) else type(d_step).__name__
        raise ValueError(f"Head.adam_step_dev: d_step must be an int32 tensor of one element on {device}, got {got}")


def check_forward_routes(in_dim, classes, device, emb, route_slot, route_head, rows_per_slot, n_slots, out=None, invalid=None):
    """What HeadGroup.forward_routes refuses, decided before any device call: emb a contiguous float32 [B, in_dim], route_slot and
    route_head contiguous int32 vectors of one length, `out` (if given) a contiguous float32 [n_routes, rows_per_slot, classes], `invalid`
    (if given) an int32 [1], all on `device`; rows_per_slot and n_slots not negative.  -> (B, n_routes).  ValueError otherwise."""
    import torch
    if not torch.is_tensor(emb) or emb.dim() != 2 or emb.shape[1] != in_dim or emb.dtype != torch.float32 or not emb.is_contiguous() or emb.device != device:
        raise ValueError(f"HeadGroup.forward_routes takes a contiguous float32 emb [B, {in_dim}] on {device}")
    for name, t in (("route_slot", route_slot), ("route_head", route_head)):
        if not torch.is_tensor(t) or t.dtype != torch.int32 or t.dim() != 1 or not t.is_contiguous() or t.device != device:
            raise ValueError(f"HeadGroup.forward_routes: {name} must be a contiguous int32 vector on {device}")
    R = int(route_slot.shape[0])
    if int(route_head.shape[0]) != R:
        raise ValueError(f"HeadGroup.forward_routes: {int(route_head.shape[0])} head indices for {R} routes")
    if int(rows_per_slot) < 0 or int(n_slots) < 0:
        raise ValueError(f"HeadGroup.forward_routes: rows_per_slot={rows_per_slot}, n_slots={n_slots}")
    if out is not None and (not torch.is_tensor(out) or tuple(out.shape) != (R, int(rows_per_slot), classes) or out.dtype != torch.float32
                            or not out.is_contiguous() or out.device != device):
        raise ValueError(f"HeadGroup.forward_routes: out must be a contiguous float32 [{R}, {int(rows_per_slot)}, {classes}] on {device}")
    if invalid is not None and (not torch.is_tensor(invalid) or invalid.numel() != 1 or invalid.dtype != torch.int32 or invalid.device != device):
        raise ValueError(f"HeadGroup.forward_routes: invalid must be an int32 [1] on {device}")
    return int(emb.shape[0]), R


class HeadGroup:
    """Several Heads of equal dimensions stepped side by side (mkws_head_group_*, include/mkws.h): one launch per stage for all of
    them instead of four small dependent launches per head.  Every head computes what Head.loss_grad + Head.adam_step compute on it
    alone, bit for bit, and stays an ordinary Head; closing the group leaves the heads alive (close the group first)."""

    def __init__(self, heads):
        import torch
        self.heads = list(heads)           # also keeps them alive: the group holds device pointers into them
        self.L = _lib.lib()
        self.h = None
        if any(getattr(hd, "h", None) is None for hd in self.heads):
            raise ValueError("HeadGroup: a head is closed")
        if len({hd.device for hd in self.heads}) > 1:
            raise ValueError("HeadGroup: the heads live on different devices")
        self.device = self.heads[0].device if self.heads else torch.device(f"cuda:{torch.cuda.current_device()}")
        table = (ctypes.c_void_p * max(len(self.heads), 1))(*[hd.h.value for hd in self.heads])
        g = ctypes.c_void_p()
        with torch.cuda.device(self.device):
            _lib.check(self.L.mkws_head_group_create(table, len(self.heads), ctypes.byref(g)))
        self.h = g
        self.generation = _lib.next_generation()
        self.in_dim = self.heads[0].in_dim
        self._stats = torch.zeros((len(self.heads), 2), dtype=torch.float32, device=self.device)

    def __len__(self):
        return len(self.heads)

    def close(self):
        if getattr(self, "h", None):
            self.L.mkws_head_group_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def forward_segments(self, emb, seg_offsets, seg_head, row_base=0, out=None, invalid=None):
        """The group as a head table (mkws_head_group_forward_segments): emb CUDA float32 [B, in] is one batch of a concatenation of
        segments, its first row being global row `row_base`; segment s = global rows seg_offsets[s] .. seg_offsets[s + 1] (CUDA int32
        [S + 1], non-decreasing: the caller checks, detector.check_segments) under member seg_head[s] (CUDA int32 [S]).
        -> (probs CUDA [B, classes] -- `out` if given --, invalid CUDA int32 [1] -- `invalid` if given).  A row's probabilities are
        Head.forward's of its head, bit for bit; rows in no segment or under a head index outside the group are NaN and counted in
        `invalid`.  Asynchronous: nothing is copied and nothing synchronises."""
        import torch
        classes = self.heads[0].classes
        if emb.dim() != 2 or emb.shape[1] != self.in_dim or emb.dtype != torch.float32 or not emb.is_contiguous() or emb.device != self.device:
            raise ValueError(f"HeadGroup.forward_segments takes a contiguous float32 emb [B, {self.in_dim}] on {self.device}, got {tuple(emb.shape)}")
        for name, t in (("seg_offsets", seg_offsets), ("seg_head", seg_head)):
            if not torch.is_tensor(t) or t.dtype != torch.int32 or t.dim() != 1 or not t.is_contiguous() or t.device != self.device:
                raise ValueError(f"HeadGroup.forward_segments: {name} must be a contiguous int32 vector on {self.device}")
        S = seg_head.shape[0]
        if seg_offsets.shape[0] != S + 1:
            raise ValueError(f"HeadGroup.forward_segments: {seg_offsets.shape[0]} offsets for {S} segments (S + 1 expected)")
        B = emb.shape[0]
        probs = out if out is not None else torch.empty((B, classes), dtype=torch.float32, device=self.device)
        if tuple(probs.shape) != (B, classes) or probs.dtype != torch.float32 or not probs.is_contiguous() or probs.device != self.device:
            raise ValueError(f"HeadGroup.forward_segments: out must be a contiguous float32 [{B}, {classes}] on {self.device}")
        bad = invalid if invalid is not None else torch.zeros(1, dtype=torch.int32, device=self.device)
        if bad.numel() != 1 or bad.dtype != torch.int32 or bad.device != self.device:
            raise ValueError(f"HeadGroup.forward_segments: invalid must be an int32 [1] on {self.device}")
        with torch.cuda.device(self.device):
            _lib.check(self.L.mkws_head_group_forward_segments(self.h, ctypes.c_void_p(emb.data_ptr()), B, int(row_base), ctypes.c_void_p(seg_offsets.data_ptr()),
                                                               ctypes.c_void_p(seg_head.data_ptr()), S, ctypes.c_void_p(probs.data_ptr()),
                                                               ctypes.c_void_p(bad.data_ptr()), _lib.current_stream_ptr()))
        return probs, bad

    def forward_routes(self, emb, route_slot, route_head, rows_per_slot, n_slots, out=None, invalid=None):
        """The group as a head table behind a ROUTE table (mkws_head_group_forward_routes): emb CUDA float32 [B, in] holds rows_per_slot
        rows per slot; route r = member route_head[r] on the rows of slot route_slot[r] (CUDA int32 [R] each; the kernel reads them, so they
        may be rewritten between calls or replays).  -> (probs CUDA [R, rows_per_slot, classes] -- `out` if given --, invalid CUDA int32
        [1] -- `invalid` if given).  A row's probabilities are Head.forward's of its head on that embedding row, bit for bit; a route with
        slot < 0 is disabled (its rows are not written); one with a slot >= n_slots, a head index outside the group or rows past B gets NaN
        rows and is counted in `invalid`.  Asynchronous: nothing is copied and nothing synchronises."""
        import torch
        classes = self.heads[0].classes
        B, R = check_forward_routes(self.in_dim, classes, self.device, emb, route_slot, route_head, rows_per_slot, n_slots, out, invalid)
        probs = out if out is not None else torch.empty((R, int(rows_per_slot), classes), dtype=torch.float32, device=self.device)
        bad = invalid if invalid is not None else torch.zeros(1, dtype=torch.int32, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(self.L.mkws_head_group_forward_routes(self.h, ctypes.c_void_p(emb.data_ptr()), B, int(rows_per_slot), int(n_slots),
                                                             ctypes.c_void_p(route_slot.data_ptr()), ctypes.c_void_p(route_head.data_ptr()), R,
                                                             ctypes.c_void_p(probs.data_ptr()), ctypes.c_void_p(bad.data_ptr()), _lib.current_stream_ptr()))
        return probs, bad

    def loss_grad(self, emb, labels, rows=None, offset=0):
        """Head k takes rows [offset, offset + rows) of emb[k] (CUDA float32 [K, R, in], contiguous) with labels[k] (CUDA int32
        [K, R], contiguous); nothing is copied, the stride between heads is the tensors'.  Returns a CUDA [K, 2] tensor of
        {sum of row losses, number correct} per head that the next call rewrites (asynchronous; .tolist() syncs)."""
        import torch
        K = len(self.heads)
        if emb.dim() != 3 or labels.dim() != 2 or emb.shape[0] != K or labels.shape[0] != K or emb.shape[2] != self.in_dim:
            raise ValueError(f"HeadGroup.loss_grad: emb {tuple(emb.shape)} / labels {tuple(labels.shape)} for {K} heads of {self.in_dim} inputs")
        if emb.dtype != torch.float32 or labels.dtype != torch.int32 or not emb.is_contiguous() or not labels.is_contiguous():
            raise ValueError("HeadGroup.loss_grad takes a contiguous float32 emb and a contiguous int32 labels tensor (no copies are made here)")
        if emb.device != self.device or labels.device != self.device:
            raise ValueError(f"HeadGroup.loss_grad: tensors must live on {self.device}")
        R = emb.shape[1]
        rows = R - int(offset) if rows is None else int(rows)
        offset = int(offset)
        if offset < 0 or rows <= 0 or offset + rows > R or offset + rows > labels.shape[1]:
            raise ValueError(f"HeadGroup.loss_grad: rows [{offset}, {offset + rows}) outside the {R} rows of emb / {labels.shape[1]} of labels")
        x = emb.data_ptr() + 4 * offset * self.in_dim
        y = labels.data_ptr() + 4 * offset
        with torch.cuda.device(self.device):
            _lib.check(self.L.mkws_head_group_loss_grad(self.h, ctypes.c_void_p(x), emb.stride(0), ctypes.c_void_p(y), labels.stride(0), rows,
                                                        ctypes.c_void_p(self._stats.data_ptr()), _lib.current_stream_ptr()))
        return self._stats

    def adam_step(self, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-7, grad_scale=1.0):
        """Head.adam_step of every member; they must stand at the same step index."""
        import torch
        ts = {hd.step_t for hd in self.heads}
        if len(ts) != 1:
            raise ValueError(f"HeadGroup.adam_step: the heads stand at different Adam steps {sorted(ts)}")
        t = ts.pop() + 1
        with torch.cuda.device(self.device):
            _lib.check(self.L.mkws_head_group_adam_step(self.h, lr, beta1, beta2, eps, t, grad_scale, _lib.current_stream_ptr()))
        for hd in self.heads:
            hd.step_t = t
