"""The handle the training-operator tests (test_train_gpu.py, test_train_routes_gpu.py) call the mkws_op_* C-ABI through."""
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
