"""The handle the training-operator tests (test_train_gpu.py, test_train_routes_gpu.py, test_train_arena_gpu.py) call the mkws_op_* C-ABI through,
and the fenced buffers of test_train_arena_gpu.py."""
import ctypes

import numpy as np


def make_ops():
    import torch
    from multilingual_kws_amd import _lib
    L = _lib.lib()
    dev = torch.device("cuda:0")

    class Ops:
        pass
    o = Ops()
    o.L, o.dev, o.check, o.s = L, dev, _lib.check, _lib.current_stream_ptr
    o.p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
    o.t = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32)).to(dev)
    # scratch arena for the partial sums of the fixed-order reductions (include/mkws.h: mkws_op_set_scratch)
    o.scratch = torch.empty(4 << 20, dtype=torch.float32, device=dev)
    _lib.check(L.mkws_op_set_scratch(o.p(o.scratch), o.scratch.numel()))
    return o


# ---- fenced buffers (tests/test_train_arena_gpu.py): the canary word and pad size of tests/test_guard_bands_gpu.py -------------------------
CANARY = 0x7FC00BAD    # a quiet NaN: a read of a pad or of an unwritten slot poisons the result, a store over it is seen
PAD = 1 << 15          # floats in front of and behind every fenced buffer


class Fenced:
    """One CUDA allocation [PAD | n | PAD]: `whole` is its int32 view, `mid` the float32 view of the n floats in between."""

    def __init__(self, whole, n):
        import torch
        self.whole, self.n = whole, n
        self.mid = whole[PAD:PAD + n].view(torch.float32)

    def pads_intact(self):
        return bool((self.whole[:PAD] == CANARY).all()) and bool((self.whole[PAD + self.n:] == CANARY).all())

    def untouched(self):
        """pads and middle still hold the canary"""
        return bool((self.whole == CANARY).all())


def fenced(n, fill=None):
    """[PAD | n | PAD] with canary pads.  fill = None: the middle is the NaN canary too (arenas, outputs); otherwise the middle holds `fill`
    (a numpy array or a tensor of n values: inputs, and outputs an operator updates in place)."""
    import torch
    n = int(n)
    f = Fenced(torch.full((PAD + n + PAD,), CANARY, dtype=torch.int32, device="cuda"), n)
    if fill is not None:
        src = fill if isinstance(fill, torch.Tensor) else torch.as_tensor(np.ascontiguousarray(fill, dtype=np.float32))
        f.mid.copy_(src.reshape(-1).to(torch.float32))
    return f


def pads_intact(*buffers):
    return all(b.pads_intact() for b in buffers)


class bound_arena:
    """with bound_arena(ops, floats) as arena: the thread's default context works in a fenced, NaN-filled arena of exactly `floats` floats
    (floats = 0: no arena at all, arena is None); afterwards -- also when the body raises -- the module's big arena is bound again."""

    def __init__(self, ops, floats):
        self.ops, self.floats = ops, int(floats)

    def __enter__(self):
        o = self.ops
        o.check(o.L.mkws_train_ctx_bind(None))
        if self.floats == 0:
            o.check(o.L.mkws_op_set_scratch(None, 0))
            return None
        arena = fenced(self.floats)
        o.check(o.L.mkws_op_set_scratch(o.p(arena.mid), self.floats))
        return arena

    def __exit__(self, *exc):
        o = self.ops
        o.check(o.L.mkws_train_ctx_bind(None))
        o.check(o.L.mkws_op_set_scratch(o.p(o.scratch), o.scratch.numel()))
        return False
