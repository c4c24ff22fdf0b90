"""No GPU: what every arena user of the training operators (mkws_op_*, include/mkws.h) states as its need.  A refusal comes before any device
call, so it can be asked for without a device: with no arena bound and dummy non-NULL pointers every call returns MKWS_ERR_INVALID_ARG, and the
float count in mkws_last_error() equals the formula written here in terms of the launch constants (mkws_op_get_option) and the 64-row and
32-position chunk sizes.  tests/test_train_arena_gpu.py then shows on the device that the kernels stay inside these counts.

mkws_op_gemm with ksplit = 0 is absent on purpose: its automatic split follows the arena and is never refused (without an arena it does not
split and goes straight to the device)."""
import ctypes
import re

import pytest

from multilingual_kws_amd import _lib

INVALID_ARG = -1
OPERAND_FLOATS = 2 << 20              # the largest operand of any case below is the [bn_chunk_cap * 128 + 1, 100] activation
EPS = 1e-3


def _ceil(a, b):
    return (a + b - 1) // b


def _r64(v):
    return (v + 63) // 64 * 64


@pytest.fixture(scope="module")
def L():
    lib = _lib.lib()
    _lib.check(lib.mkws_train_ctx_bind(None))
    _lib.check(lib.mkws_op_set_scratch(None, 0))
    return lib


@pytest.fixture(scope="module")
def P():
    """The one pointer every operand of every call is: a dummy -- the host never dereferences it and no launch may happen.  Where the suite runs
    on a machine with a device it is a real buffer that holds the largest operand, so that a launch that must not happen fails this test
    (wrong return code) without touching memory that is not ours."""
    try:
        import torch
        if torch.cuda.is_available():
            buf = torch.zeros(OPERAND_FLOATS, dtype=torch.float32, device="cuda")
            yield ctypes.c_void_p(buf.data_ptr())
            torch.cuda.synchronize()
            return
    except ImportError:
        pass
    yield ctypes.c_void_p(0x10000)


@pytest.fixture(scope="module")
def c(L):
    k = {name: L.mkws_op_get_option(name.encode()) for name in ("bn_small_rows", "bn_chunk_cap", "bn_max_chunks", "bn_max_gemm_tiles")}
    assert all(v > 0 for v in k.values()), k
    return k


def bn_need(c, M, C):
    """statistics / backward-reduce launches: chunks of 128 rows, at most bn_chunk_cap of them; (mean, M2) or two sums per chunk and channel"""
    return min(_ceil(M, 128), c["bn_chunk_cap"]) * 2 * C


def dw_bwd_need(B, Ho, Wo, C, k):
    """chunks of 32 output positions, capped at min(ceil(512 / slabs of 16 channel quads), 256); k * k * C sums per chunk"""
    xb = _ceil(C // 4, 16)
    return min(_ceil(B * Ho * Wo, 32), min(_ceil(512, xb), 256)) * k * k * C


def se_need(B, C, se):
    """batch chunks of 64 clips; dWr and dWe partials, then dbe, then dbr, each rounded up to 64 floats (one chunk: direct stores, no arena)"""
    chunks = _ceil(B, 64)
    return 0 if chunks == 1 else 2 * _r64(chunks * se * C) + _r64(chunks * C) + _r64(chunks * se)


def dscnn_stem_need(B):
    """a wave walks a multiple of four pixels, at least 16, in at most 256 workgroups of four waves; [40 taps, 64 channels] per workgroup"""
    npix = B * 500
    target = min(_ceil(npix, 64), 256)
    wave_px = (_ceil(npix, 4 * target) + 3) // 4 * 4
    return _ceil(npix, 4 * wave_px) * 40 * 64


def _cases(c, P):
    capM = c["bn_chunk_cap"] * 128 + 1
    small1 = c["bn_small_rows"] + 1
    assert capM * 100 <= OPERAND_FLOATS and 300 * 2048 <= OPERAND_FLOATS
    Bdw = c["bn_max_chunks"] * 128 // 4 + 1                       # 2 x 2 images: one clip above bn_max_chunks chunks of 128 rows
    out = []
    for M, C in ((300, 24), (capM, 100)):
        out += [(f"bn_stats {M}x{C}", lambda L, M=M, C=C: L.mkws_op_bn_stats(P, M, C, P, P, None), bn_need(c, M, C)),
                (f"bn_train_fwd {M}x{C}", lambda L, M=M, C=C: L.mkws_op_bn_train_fwd(P, M, C, P, P, EPS, 1, 0.99, P, P, P, P, P, None), bn_need(c, M, C)),
                (f"bn_train_fwd_res {M}x{C}", lambda L, M=M, C=C: L.mkws_op_bn_train_fwd_res(P, M, C, P, P, EPS, 1, 0.99, P, P, P, P, P, P, P, 35, None),
                 bn_need(c, M, C))]
    out += [
        ("bn_act_bwd_ex", lambda L: L.mkws_op_bn_act_bwd_ex(P, P, P, P, P, EPS, 1, P, P, P, P, 0.5, 35, P, P, small1, 40, None), bn_need(c, small1, 40)),
        # the sequence route's need decides the refusal (the fused route's ceil(M / 64) * 2 * N only selects the route)
        ("conv_bn_fwd", lambda L: L.mkws_op_conv_bn_fwd(P, P, P, 130, 24, 16, P, P, EPS, 1, 0.99, P, P, P, P, P, None, None, 1, None), bn_need(c, 130, 24)),
        # up to bn_max_chunks chunks of 128 output rows the convolution leaves one (mean, M2) per chunk; above, the statistics launch's chunks
        ("dwconv_bn_fwd", lambda L: L.mkws_op_dwconv_bn_fwd(P, P, P, 5, 7, 5, 40, 3, 1, 1, 1, 7, 5, P, P, EPS, 1, 0.99, P, P, P, P, P, None),
         _ceil(5 * 7 * 5, 128) * 2 * 40),
        ("dwconv_bn_fwd sequence", lambda L: L.mkws_op_dwconv_bn_fwd(P, P, P, Bdw, 2, 2, 8, 3, 1, 1, 1, 2, 2, P, P, EPS, 1, 0.99, P, P, P, P, P, None),
         bn_need(c, Bdw * 4, 8)),
        ("dwconv_bwd", lambda L: L.mkws_op_dwconv_bwd(P, P, P, None, P, 5, 7, 5, 40, 5, 1, 2, 2, 7, 5, None), dw_bwd_need(5, 7, 5, 40, 5)),
        ("dwconv_bwd dX+dW", lambda L: L.mkws_op_dwconv_bwd(P, P, P, P, P, 5, 7, 5, 40, 5, 1, 2, 2, 7, 5, None), dw_bwd_need(5, 7, 5, 40, 5)),
        ("dwconv_bwd capped", lambda L: L.mkws_op_dwconv_bwd(P, P, P, None, P, 41, 20, 10, 8, 3, 1, 1, 1, 20, 10, None), dw_bwd_need(41, 20, 10, 8, 3)),
        ("se_wgrad", lambda L: L.mkws_op_se_wgrad(P, P, P, P, P, P, P, P, 65, 40, 10, None), se_need(65, 40, 10)),
        ("se_bwd_fused", lambda L: L.mkws_op_se_bwd_fused(*([P] * 17), 65, 12, 40, 10, None), se_need(65, 40, 10)),
        ("bias_act_bwd", lambda L: L.mkws_op_bias_act_bwd(P, P, 1, P, P, 130, 10, None), min(_ceil(130, 64), 64) * 10),
        # explicit ksplit: one [M, N] slab of slice sums per slice
        ("gemm TN ksplit 7", lambda L: L.mkws_op_gemm(P, P, P, 16, 96, 4000, 16, 96, 96, 1, 0, 0, 7, None), 7 * 16 * 96),
        ("gemm NN ksplit 4", lambda L: L.mkws_op_gemm(P, P, P, 300, 96, 2048, 2048, 96, 96, 0, 0, 0, 4, None), 4 * 300 * 96),
        ("gemm NN ksplit 3", lambda L: L.mkws_op_gemm(P, P, P, 33, 65, 1000, 1000, 65, 65, 0, 0, 0, 3, None), 3 * 33 * 65),
    ]
    for B in (1, 3):
        # workgroups of 256 pixels, at most 256; [9 taps, 32 channels] per workgroup
        out += [(f"stem_bwd_weight B={B}", lambda L, B=B: L.mkws_op_stem_bwd_weight(P, P, 0.1, 0.7, P, B, None), min(_ceil(B * 500, 256), 256) * 288),
                (f"dscnn_stem_bwd_weight B={B}", lambda L, B=B: L.mkws_op_dscnn_stem_bwd_weight(P, P, P, B, None), dscnn_stem_need(B))]
    return out


def test_formulas_at_the_shapes_of_the_device_tests(c):
    """the constants as shipped give these counts (a retune changes them here and in the library together)"""
    if (c["bn_small_rows"], c["bn_chunk_cap"], c["bn_max_chunks"]) == (1024, 128, 256):
        assert bn_need(c, 300, 24) == 144 and bn_need(c, 16385, 100) == 25600 and bn_need(c, 1025, 40) == 720
    assert dw_bwd_need(5, 7, 5, 40, 5) == 6 * 25 * 40 and dw_bwd_need(41, 20, 10, 8, 3) == 256 * 9 * 8
    assert se_need(64, 40, 10) == 0 and se_need(65, 40, 10) == 2 * 832 + 128 + 64
    assert dscnn_stem_need(1) == 8 * 2560 and dscnn_stem_need(3) == 24 * 2560


def test_every_arena_user_states_its_need_and_refuses_before_any_device_call(L, c, P):
    cases = _cases(c, P)
    for name, call, need in cases:
        _lib.check(L.mkws_op_set_scratch(None, 0))
        rc = call(L)
        msg = L.mkws_last_error().decode()
        assert rc == INVALID_ARG, (name, rc, msg)
        m = re.search(r"(\d+) floats", msg)
        assert "scratch" in msg and m, (name, msg)
        assert int(m.group(1)) == need, (name, msg, need)

