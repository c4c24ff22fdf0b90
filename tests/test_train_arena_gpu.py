"""-m gpu: the training operators (mkws_op_*) inside a tight, fenced, NaN-filled scratch arena -- the tripwire tests/test_guard_bands_gpu.py is for
the embedding forward pass.  Every other test hands the operators 4 Mi floats of whatever the allocator left; here the arena holds exactly the
floats a call states as its need (tests/test_train_arena_cpu.py pins those counts to their formulas), starts as a NaN canary and lies between
two canary pads, like every input and output of the call:

  (a) an operator asks for what it uses: refused without an arena and with one float too few, with every output untouched; in exactly `need`
      floats it keeps every fence, and its outputs are finite and equal, bit for bit, those of the same call in the big arena -- also when the
      arena is dirty from the call before;
  (b) the automatic split of mkws_op_gemm follows the arena size;
  (c) deferred folds are flushed when the arena fills, with the same bits;
  (d) one whole step of each trainer in fenced, NaN-filled arenas equals the step of a twin on ordinary ones.

Bounds against float64 are the ones an existing test holds the same operator to (named where they are used); every other comparison is a
bit-equality between two runs of the same route."""
import re
import types

import numpy as np
import pytest

from tests.util_train_ops import bound_arena, fenced, make_ops

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
INVALID_ARG = -1
EPS = 1e-3


def _ceil(a, b):
    return (a + b - 1) // b


def _r64(v):
    return _ceil(v, 64) * 64


def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-30))


@pytest.fixture(scope="module")
def ops():
    return make_ops()


@pytest.fixture(scope="module")
def c(ops):
    k = types.SimpleNamespace()
    for name in ("bn_small_rows", "bn_chunk_cap", "bn_max_chunks", "bn_max_gemm_tiles"):
        v = ops.L.mkws_op_get_option(name.encode())
        assert v > 0, name
        setattr(k, name, v)
    return k


@pytest.fixture(autouse=True)
def _big_arena(ops):
    ops.check(ops.L.mkws_train_ctx_bind(None))
    ops.check(ops.L.mkws_op_set_scratch(ops.p(ops.scratch), ops.scratch.numel()))
    yield
    ops.check(ops.L.mkws_train_ctx_bind(None))
    ops.check(ops.L.mkws_op_set_scratch(ops.p(ops.scratch), ops.scratch.numel()))


# ---------------------------------------------------------------------------------------------------------------------------------------------
# one operator call on fenced buffers of its own
class Call:
    def __init__(self, ops):
        self.ops, self.ins, self.outs, self.fn = ops, [], [], None

    def i(self, a):
        """an input: data between two NaN pads"""
        f = fenced(a.size, a)
        self.ins.append(f)
        return self.ops.p(f.mid)

    def o(self, n, init=None):
        """an output: the NaN canary between two canary pads (init: the data of a buffer the operator updates in place)"""
        f = fenced(n, init)
        self.outs.append(f)
        return self.ops.p(f.mid)

    def snapshot(self):
        return [f.whole.clone() for f in self.ins + self.outs]

    def run(self):
        rc = self.fn()
        msg = self.ops.L.mkws_last_error().decode() if rc else ""
        torch.cuda.synchronize()
        return rc, msg


def _bits(t):
    return t.view(torch.int32)


def _reference(ops, make):
    """the call on the ordinary 4 Mi arena"""
    ref = make(ops)
    rc, msg = ref.run()
    assert rc == 0, msg
    assert all(bool(torch.isfinite(f.mid).all()) for f in ref.outs)
    return ref


def _refused(ops, make, floats):
    """floats = 0: no arena.  MKWS_ERR_INVALID_ARG, the message names `scratch` and the need, and nothing was launched: every buffer is as it was"""
    k = make(ops)
    before = k.snapshot()
    with bound_arena(ops, floats) as arena:
        rc, msg = k.run()
    m = re.search(r"(\d+) floats", msg)
    assert rc == INVALID_ARG and "scratch" in msg and m, (floats, rc, msg)
    names = [f"input {n}" for n in range(len(k.ins))] + [f"output {n}" for n in range(len(k.outs))]
    written = [name for name, f, b in zip(names, k.ins + k.outs, before) if not torch.equal(f.whole, b)]
    assert not written, f"a call refused with {floats} floats of arena has written {written}"
    assert arena is None or arena.untouched(), "a refused call has written the arena"
    return int(m.group(1))


def _same(k, ref, arena, before, what):
    fence = arena is None or arena.pads_intact()
    assert fence, f"{what}: a store outside the floats the call asked for"
    written = [n for n, (f, b) in enumerate(zip(k.ins, before)) if not torch.equal(f.whole, b)]
    assert not written, f"{what}: inputs {written} or their surroundings were written"
    for n, (f, r) in enumerate(zip(k.outs, ref.outs)):
        fence, finite, same = f.pads_intact(), bool(torch.isfinite(f.mid).all()), torch.equal(_bits(f.mid), _bits(r.mid))
        assert fence, f"{what}: a store outside output {n}"
        assert finite, f"{what}: output {n} holds a NaN: a slot of the arena, or a pad, was read before it was written"
        assert same, f"{what}: output {n} depends on what the arena held"


def _runs_in(ops, make, floats, ref):
    """two calls in one fenced arena of `floats` floats (0: none): NaN-filled, then dirty"""
    with bound_arena(ops, floats) as arena:
        for state in ("NaN-filled arena", "dirty arena"):
            k = make(ops)
            before = k.snapshot()
            rc, msg = k.run()
            assert rc == 0, (state, floats, msg)
            _same(k, ref, arena, before, f"{state} of {floats} floats")


def protocol(ops, make, formula=None):
    ref = _reference(ops, make)
    need = _refused(ops, make, 0)
    assert _refused(ops, make, need - 1) == need
    _runs_in(ops, make, need, ref)
    if formula is not None:                                       # (tests/test_train_arena_cpu.py holds every stated need to its formula without a device)
        assert need == formula, (need, formula)
    return need


def needs_no_arena(ops, make):
    _runs_in(ops, make, 0, _reference(ops, make))


def _channels(rng, M, C, offset=1.0, lo=0.2, hi=3.0):
    return (rng.standard_normal((M, C)) * rng.uniform(lo, hi, C) + offset * rng.standard_normal(C)).astype(np.float32)


def _affine(rng, C):
    return rng.uniform(0.5, 1.5, C).astype(np.float32), (0.1 * rng.standard_normal(C)).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# (a) BatchNorm
def bn_need(c, M, C):
    return min(_ceil(M, 128), c.bn_chunk_cap) * 2 * C


BN_SHAPES = {"300x24": lambda c: (300, 24),                                  # three chunks, the last of 44 rows; 6 live channel quads of a 64-channel slab
             "cap+1x100": lambda c: (c.bn_chunk_cap * 128 + 1, 100)}         # the cap binds: chunks of 129 rows, the last one nearly empty; a slab of 36 channels


def _bn_make(op, M, C):
    def make(ops):
        L, k, rng = ops.L, Call(ops), np.random.default_rng(M + C)
        Z = k.i(_channels(rng, M, C))
        gamma, beta = _affine(rng, C)
        if op == "bn_stats":
            mean, var = k.o(C), k.o(C)
            k.fn = lambda: L.mkws_op_bn_stats(Z, M, C, mean, var, ops.s())
            return k
        g, b = k.i(gamma), k.i(beta)
        mm, mv, mean, var, A = k.o(C, np.zeros(C)), k.o(C, np.ones(C)), k.o(C), k.o(C), k.o(M * C)
        if op == "bn_train_fwd":
            k.fn = lambda: L.mkws_op_bn_train_fwd(Z, M, C, g, b, EPS, 1, 0.99, mm, mv, mean, var, A, ops.s())
        else:
            group = 35
            res, keep = k.i(_channels(rng, M, C)), k.i(((rng.random(_ceil(M, group)) > 0.3) / 0.7).astype(np.float32))
            k.fn = lambda: L.mkws_op_bn_train_fwd_res(Z, M, C, g, b, EPS, 1, 0.99, mm, mv, mean, var, A, res, keep, group, ops.s())
        return k
    return make


@pytest.mark.parametrize("shape", list(BN_SHAPES))
@pytest.mark.parametrize("op", ["bn_stats", "bn_train_fwd", "bn_train_fwd_res"])
def test_batchnorm_forward_asks_for_what_it_uses(ops, c, op, shape):
    M, C = BN_SHAPES[shape](c)
    assert _ceil(M, 128) >= 2 and C % 64 != 0
    protocol(ops, _bn_make(op, M, C), bn_need(c, M, C))


def _bn_bwd_make(M, C):
    def make(ops):
        k, rng, group = Call(ops), np.random.default_rng(M), 35
        z = _channels(rng, M, C)
        gamma, beta = _affine(rng, C)
        Z, mean, var = k.i(z), k.i(z.mean(0)), k.i(z.var(0))
        g, b = k.i(gamma), k.i(beta)
        src, keep = k.i(rng.standard_normal((M, C)).astype(np.float32)), k.i(((rng.random(_ceil(M, group)) > 0.3) / 0.7).astype(np.float32))
        bc = k.i(rng.standard_normal((_ceil(M, group), C)).astype(np.float32))
        dA, dg, db = k.o(M * C), k.o(C), k.o(C)
        k.fn = lambda: ops.L.mkws_op_bn_act_bwd_ex(Z, mean, var, g, b, EPS, 1, dA, src, keep, bc, 1.0 / group, group, dg, db, M, C, ops.s())
        return k
    return make


def test_batchnorm_backward_asks_for_what_it_uses(ops, c):
    C = 40
    M = c.bn_small_rows + 1                                       # the first M of the two-launch route
    assert _ceil(M, 128) >= 2
    protocol(ops, _bn_bwd_make(M, C), bn_need(c, M, C))
    needs_no_arena(ops, _bn_bwd_make(c.bn_small_rows, C))         # the one-launch kernel: no partial sums leave the workgroup


# ---------------------------------------------------------------------------------------------------------------------------------------------
# (a) 1x1 convolution + BatchNorm: the arena size picks the route
def _conv_bn_make(M, K, N, data):
    def make(ops):
        k = Call(ops)
        X, W, g, b = (k.i(data[n]) for n in ("X", "W", "gamma", "beta"))
        Z, mm, mv, mean, var, A = k.o(M * N), k.o(N, np.zeros(N)), k.o(N, np.ones(N)), k.o(N), k.o(N), k.o(M * N)
        k.fn = lambda: ops.L.mkws_op_conv_bn_fwd(X, W, Z, M, N, K, g, b, EPS, 1, 0.99, mm, mv, mean, var, A, None, None, 1, ops.s())
        return k
    return make


def test_conv_batchnorm_route_follows_the_arena(ops, c):
    M, K, N = 130, 16, 24
    fused_need, seq_need = _ceil(M, 64) * 2 * N, bn_need(c, M, N)      # one chunk per 64-row GEMM tile / per 128 rows of the statistics launch
    assert _ceil(M, 64) <= c.bn_max_gemm_tiles and seq_need < fused_need
    rng = np.random.default_rng(M)
    data = {"X": _channels(rng, M, K, lo=0.5, hi=1.5, offset=0.3), "W": (rng.standard_normal((K, N)) / np.sqrt(K)).astype(np.float32)}
    data["gamma"], data["beta"] = _affine(rng, N)
    make = _conv_bn_make(M, K, N, data)
    ref = _reference(ops, make)
    # below the smaller need: refused, Z (and everything else) untouched; the message states the smaller need
    assert _refused(ops, make, 0) == seq_need and _refused(ops, make, seq_need - 1) == seq_need
    # exactly the fused need: the route of the big arena, bit for bit
    _runs_in(ops, make, fused_need, ref)
    # between the two needs: the three-launch sequence.  Against float64 at the bounds of test_conv_batchnorm_as_one_operator (tests/test_train_gpu.py):
    # mean (absolute), variance, moving statistics 1e-5, output 1e-4; Z is the same GEMM launch: the same bits
    z = data["X"].astype(np.float64) @ data["W"].astype(np.float64)
    mean, var = z.mean(0), z.var(0)
    y = torch.from_numpy(data["gamma"] * (z - mean) / np.sqrt(var + EPS) + data["beta"])
    a = (y * torch.sigmoid(y)).numpy()
    for floats in (seq_need, fused_need - 1):
        with bound_arena(ops, floats) as arena:
            for state in ("NaN-filled", "dirty"):
                k = make(ops)
                before = k.snapshot()
                rc, msg = k.run()
                assert rc == 0, (floats, state, msg)
                assert arena.pads_intact() and all(f.pads_intact() for f in k.outs), (floats, state)
                assert all(torch.equal(f.whole, b) for f, b in zip(k.ins, before))
                Z, mm, mv, m1, v1, A = (f.mid.cpu().numpy() for f in k.outs)
                assert np.array_equal(Z.view(np.uint32), ref.outs[0].mid.cpu().numpy().view(np.uint32))
                errs = {"mean": float(np.abs(m1 - mean).max()), "var": _rel(v1, var), "moving mean": _rel(mm, 0.01 * mean),
                        "moving var": _rel(mv, 0.99 + 0.01 * var * M / (M - 1)), "out": _rel(A.reshape(M, N), a)}
                print(f"conv + BN in {floats} floats ({state}):", {n: f"{v:.2e}" for n, v in errs.items()})
                assert all(np.isfinite(v) and v < (1e-4 if n == "out" else 1e-5) for n, v in errs.items()), errs


# ---------------------------------------------------------------------------------------------------------------------------------------------
# (a) depthwise convolution + BatchNorm, depthwise weight gradient
def _dw_bn_make(B, H, W, C, k_, s):
    def make(ops):
        k, rng, M = Call(ops), np.random.default_rng(B + C), B * H * W
        X, Wt = k.i(_channels(rng, M, C, lo=0.5, hi=2.0)), k.i((rng.standard_normal((k_, k_, C)) / k_).astype(np.float32))
        gamma, beta = _affine(rng, C)
        g, b = k.i(gamma), k.i(beta)
        Z, mm, mv, mean, var, A = k.o(M * C), k.o(C, np.zeros(C)), k.o(C, np.ones(C)), k.o(C), k.o(C), k.o(M * C)
        k.fn = lambda: ops.L.mkws_op_dwconv_bn_fwd(X, Wt, Z, B, H, W, C, k_, s, k_ // 2, k_ // 2, H, W, g, b, EPS, 1, 0.99, mm, mv, mean, var, A, ops.s())
        return k
    return make


def test_depthwise_batchnorm_asks_for_what_it_uses(ops, c):
    B, H, W, C = 5, 7, 5, 40
    assert 2 <= _ceil(B * H * W, 128) <= c.bn_max_chunks         # the convolution leaves one (mean, M2) per chunk of 128 output rows
    protocol(ops, _dw_bn_make(B, H, W, C, 3, 1), _ceil(B * H * W, 128) * 2 * C)


def test_depthwise_batchnorm_sequence_refuses_before_the_convolution(ops, c):
    """just above bn_max_chunks chunks: convolution, statistics, normalise.  The statistics' need is known before the convolution runs into Z."""
    H = W = 2
    B = c.bn_max_chunks * 128 // (H * W) + 1
    assert _ceil(B * H * W, 128) > c.bn_max_chunks and _ceil((B - 1) * H * W, 128) <= c.bn_max_chunks
    protocol(ops, _dw_bn_make(B, H, W, 8, 3, 1), bn_need(c, B * H * W, 8))


def dw_bwd_chunks(npos, C):
    xb = _ceil(C // 4, 16)
    return min(_ceil(npos, 32), min(_ceil(512, xb), 256))


def _dw_bwd_make(B, H, W, C, k_, with_dX):
    def make(ops):
        k, rng, M = Call(ops), np.random.default_rng(B * H + C), B * H * W
        X, Wt, dZ = k.i(_channels(rng, M, C, lo=0.5, hi=1.5, offset=0.3)), k.i(rng.standard_normal((k_, k_, C)).astype(np.float32)), k.i(rng.standard_normal((M, C)).astype(np.float32))
        dX = k.o(M * C) if with_dX else None
        dW = k.o(k_ * k_ * C)
        k.fn = lambda: ops.L.mkws_op_dwconv_bwd(X, Wt, dZ, dX, dW, B, H, W, C, k_, 1, k_ // 2, k_ // 2, H, W, ops.s())
        return k
    return make


@pytest.mark.parametrize("with_dX", [False, True], ids=["dW", "dX+dW"])
def test_depthwise_weight_gradient_asks_for_what_it_uses(ops, with_dX):
    """with dX asked for as well, the refusal (the weight gradient's arena) comes before the input gradient's launch: dX untouched"""
    B, H, W, C, k = 5, 7, 5, 40, 5
    assert dw_bwd_chunks(B * H * W, C) == 6 and (B * H * W) % 6 != 0
    protocol(ops, _dw_bwd_make(B, H, W, C, k, with_dX), 6 * k * k * C)


def test_depthwise_weight_gradient_with_empty_trailing_chunks(ops):
    B, H, W, C, k = 41, 20, 10, 8, 3
    npos, chunks = B * H * W, dw_bwd_chunks(B * H * W, C)
    per = _ceil(npos, chunks)
    assert chunks == 256 and _ceil(npos, 32) > 256 and per == 33   # the cap binds: 256 chunks of 33 positions each ...
    assert _ceil(npos, per) == 249 < chunks                        # ... of which the last seven hold no position: their slabs must still be written
    protocol(ops, _dw_bwd_make(B, H, W, C, k, False), chunks * k * k * C)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# (a) stem weight gradients of the two networks
def dscnn_stem_need(B):
    npix = B * 500
    target = min(_ceil(npix, 64), 256)
    wave_px = _ceil(_ceil(npix, 4 * target), 4) * 4
    return _ceil(npix, 4 * wave_px) * 40 * 64


def _stem_make(B, dscnn):
    def make(ops):
        k, rng, ch = Call(ops), np.random.default_rng(B), 64 if dscnn else 32
        spec = k.i((rng.integers(0, 670, size=(B, 49, 40)) * (10 / 256)).astype(np.float32))
        dZ = k.i(_channels(rng, B * 500, ch, lo=0.5, hi=1.5, offset=0.3))
        if dscnn:
            dW = k.o(40 * 64)
            k.fn = lambda: ops.L.mkws_op_dscnn_stem_bwd_weight(spec, dZ, dW, B, ops.s())
        else:
            dW = k.o(288)
            k.fn = lambda: ops.L.mkws_op_stem_bwd_weight(spec, dZ, 0.1, 0.7, dW, B, ops.s())
        return k
    return make


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("net", ["embedding", "dscnn"])
def test_stem_weight_gradients_ask_for_what_they_use(ops, net, B):
    need = dscnn_stem_need(B) if net == "dscnn" else min(_ceil(B * 500, 256), 256) * 288
    protocol(ops, _stem_make(B, net == "dscnn"), need)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# (a) squeeze-excite parameter gradients, alone and behind the fused backward
def se_need(B, C, se):
    chunks = _ceil(B, 64)
    return 0 if chunks == 1 else 2 * _r64(chunks * se * C) + _r64(chunks * C) + _r64(chunks * se)


def _se_wgrad_make(B, C, se):
    def make(ops):
        k, rng = Call(ops), np.random.default_rng(B + C)
        mean, R = k.i(_channels(rng, B, C, lo=0.5, hi=1.5, offset=0.3)), k.i(_channels(rng, B, se, lo=0.5, hi=1.5, offset=0.3))
        dYg, dYr = k.i(_channels(rng, B, C, lo=0.5, hi=1.5, offset=0.3)), k.i(_channels(rng, B, se, lo=0.5, hi=1.5, offset=0.3))
        dWr, dbr, dWe, dbe = k.o(C * se), k.o(se), k.o(se * C), k.o(C)
        k.fn = lambda: ops.L.mkws_op_se_wgrad(mean, R, dYg, dYr, dWr, dbr, dWe, dbe, B, C, se, ops.s())
        return k
    return make


def _se_fused_make(B, HW, C, se):
    def make(ops):
        k, rng = Call(ops), np.random.default_rng(B * HW + C)
        a = _channels(rng, B * HW, C, lo=0.5, hi=1.5, offset=0.3)
        A, G, dOut = k.i(a), k.i(rng.uniform(0.05, 0.95, (B, C)).astype(np.float32)), k.i(rng.standard_normal((B * HW, C)).astype(np.float32))
        mean, Yr = k.i(a.reshape(B, HW, C).mean(1)), k.i(rng.standard_normal((B, se)).astype(np.float32))
        R = k.i(rng.standard_normal((B, se)).astype(np.float32))
        Wr, We = k.i((rng.standard_normal((C, se)) / np.sqrt(C)).astype(np.float32)), k.i((rng.standard_normal((se, C)) / np.sqrt(se)).astype(np.float32))
        dA, dmean, dYg, dYr = k.o(B * HW * C), k.o(B * C), k.o(B * C), k.o(B * se)
        dWr, dbr, dWe, dbe = k.o(C * se), k.o(se), k.o(se * C), k.o(C)
        work = k.o(B * _ceil(C, 128) * se)                        # the caller's workspace of the gate launch: as untouched by a refused call as dA
        k.fn = lambda: ops.L.mkws_op_se_bwd_fused(A, G, dOut, mean, Yr, R, Wr, We, dA, dmean, dYg, dYr, dWr, dbr, dWe, dbe, work, B, HW, C, se, ops.s())
        return k
    return make


def test_squeeze_excite_gradients_ask_for_what_they_use(ops):
    C, se = 40, 10
    assert se_need(64, C, se) == 0 and se_need(65, C, se) == 2 * 832 + 128 + 64
    protocol(ops, _se_wgrad_make(65, C, se), se_need(65, C, se))                  # two batch chunks, the second of one clip
    protocol(ops, _se_fused_make(65, 4, C, se), se_need(65, C, se))               # a refusal leaves dA, dmean, dYg and dYr untouched
    needs_no_arena(ops, _se_wgrad_make(64, C, se))                                # one chunk: direct stores
    needs_no_arena(ops, _se_fused_make(64, 4, C, se))


# ---------------------------------------------------------------------------------------------------------------------------------------------
# (a) bias + activation backward
def test_bias_activation_backward_asks_for_what_it_uses(ops):
    M, N = 130, 10

    def make(ops):
        k, rng = Call(ops), np.random.default_rng(M + N)
        Z, bias = k.i(_channels(rng, M, N, lo=0.5, hi=1.5, offset=0.5)), k.i(rng.standard_normal(N).astype(np.float32))
        dA = k.o(M * N, _channels(rng, M, N, lo=0.5, hi=1.5, offset=0.3))         # updated in place: a refusal leaves it as it was
        dbias = k.o(N)
        k.fn = lambda: ops.L.mkws_op_bias_act_bwd(Z, bias, 1, dA, dbias, M, N, ops.s())
        return k
    protocol(ops, make, min(_ceil(M, 64), 64) * N)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# (a), (b) GEMM
def _gemm_data(M, N, K, ta, tb):
    rng = np.random.default_rng(M + N + K)
    A = rng.standard_normal((K, M) if ta else (M, K)).astype(np.float32)
    B = rng.standard_normal((N, K) if tb else (K, N)).astype(np.float32)
    return A, B


def _gemm_make(M, N, K, ta, tb, ks, data=None):
    A, B = data if data is not None else _gemm_data(M, N, K, ta, tb)

    def make(ops):
        k = Call(ops)
        a, b = k.i(A), k.i(B)
        C = k.o(M * N)
        k.fn = lambda: ops.L.mkws_op_gemm(a, b, C, M, N, K, A.shape[1], B.shape[1], N, ta, tb, 0, ks, ops.s())
        return k
    return make


@pytest.mark.parametrize("M,N,K,ta,ks", [(16, 96, 4000, 1, 7),        # weight gradient on the LDS-staged kernel, slices of 572 columns, the last of 568
                                         (300, 96, 2048, 0, 4),       # register-ring kernel (K, N % 4 == 0), ragged last row tile
                                         (33, 65, 1000, 0, 3)])       # N % 4 != 0: the staged kernel, ragged tiles both ways
def test_split_gemm_asks_for_what_it_uses(ops, M, N, K, ta, ks):
    assert ops.L.mkws_op_get_option(b"gemm_ring") == 1 and ops.L.mkws_op_get_option(b"gemm_ring_tn") == 0
    protocol(ops, _gemm_make(M, N, K, ta, 0, ks), ks * M * N)


@pytest.fixture
def ring_tn_all(ops):
    old = ops.L.mkws_op_get_option(b"gemm_ring_tn")
    ops.check(ops.L.mkws_op_set_option(b"gemm_ring_tn", 2))
    yield
    ops.check(ops.L.mkws_op_set_option(b"gemm_ring_tn", old))


def _gemm_in(ops, make, floats, ref64, same_as=None):
    """the GEMM in a fenced NaN-filled arena of `floats` floats (0: none), twice: fences, the 1e-5 * max|ref| of test_gemm_all_transposes
    (tests/test_train_gpu.py) against the float64 product, and the bits of `same_as`"""
    with bound_arena(ops, floats) as arena:
        for state in ("NaN-filled", "dirty"):
            k = make(ops)
            before = k.snapshot()
            rc, msg = k.run()
            assert rc == 0, (floats, state, msg)
            assert arena is None or arena.pads_intact(), f"{floats} floats, {state}: a store outside the arena"
            assert k.outs[0].pads_intact() and all(torch.equal(f.whole, b) for f, b in zip(k.ins, before))
            err = _rel(k.outs[0].mid.cpu().numpy().reshape(ref64.shape), ref64)
            print(f"gemm in {floats} floats ({state}): {err:.2e}")
            assert err < 1e-5
            if same_as is not None:
                assert torch.equal(_bits(k.outs[0].mid), _bits(same_as.outs[0].mid)), (floats, state)


def test_row_slice_gemm_follows_the_arena(ops, ring_tn_all):
    """the register-ring weight-gradient kernel (gemm_ring_tn = 2) slices the rows as far as the arena reaches: never refused.  With all of its
    slices it is the big arena's launch, bit for bit, inside exactly slices * M * N floats; with room for one slice it does not use the arena."""
    M, N, K = 32, 16, 70000
    blocks = _ceil(_ceil(M, 16), 2) * 1                            # two k-tiles per workgroup, one n-tile
    slices = min(_ceil(1024, blocks), _ceil(_ceil(K, 16), 64))     # ~1024 workgroups, at least 1024 rows a slice
    assert slices == 69
    A, B = _gemm_data(M, N, K, 1, 0)
    ref64 = A.T.astype(np.float64) @ B.astype(np.float64)
    make = _gemm_make(M, N, K, 1, 0, 0, (A, B))
    ref = _reference(ops, make)
    _gemm_in(ops, make, slices * M * N, ref64, same_as=ref)
    for held in (1, 3):
        _gemm_in(ops, make, held * M * N + M * N - 1, ref64)
    _gemm_in(ops, make, 0, ref64)


def test_automatic_split_follows_the_arena(ops):
    """ksplit = 0 splits only as far as the arena reaches: j * M * N + (M * N - 1) floats hold j slices, and the result is that of ksplit = j"""
    M, N, K = 16, 96, 32000
    assert ops.L.mkws_op_get_option(b"gemm_ring_tn") == 0
    A, B = _gemm_data(M, N, K, 1, 0)
    ref64 = A.T.astype(np.float64) @ B.astype(np.float64)
    auto = _gemm_make(M, N, K, 1, 0, 0, (A, B))
    explicit = {j: _reference(ops, _gemm_make(M, N, K, 1, 0, j, (A, B))) for j in (1, 2, 5)}
    assert not torch.equal(_bits(explicit[1].outs[0].mid), _bits(explicit[2].outs[0].mid))       # the splits do differ in their bits
    assert not torch.equal(_bits(explicit[2].outs[0].mid), _bits(explicit[5].outs[0].mid))
    for j in (1, 2, 5):
        _gemm_in(ops, auto, j * M * N + (M * N - 1), ref64, same_as=explicit[j])
    _gemm_in(ops, auto, 0, ref64, same_as=explicit[1])


# ---------------------------------------------------------------------------------------------------------------------------------------------
# (c) deferred folds when the arena fills
def test_deferred_folds_flush_when_the_arena_fills(ops):
    """The three operators and shapes of test_deferred_folds_are_bit_identical (tests/test_train_gpu.py), the GEMM with an explicit split so that
    the arena cannot change its route.  Eight rounds with one explicit flush after the fourth: in an arena of two and a half rounds the bump pointer
    runs out in mid-round, in an arena of the largest single need every request flushes what is queued, the big arena never flushes on its own."""
    L = ops.L
    rng = np.random.default_rng(11)
    M, K, N, ks = 4000, 24, 96, 16
    B, H, W, C, k = 8, 13, 10, 48, 3
    X, dZ = ops.t(rng.standard_normal((M, K))), ops.t(rng.standard_normal((M, N)))
    Zb, bias = ops.t(rng.standard_normal((M, N))), ops.t(rng.standard_normal(N))
    Xd, Wd, dZd = ops.t(rng.standard_normal((B * H * W, C))), ops.t(rng.standard_normal((k * k, C))), ops.t(rng.standard_normal((B * H * W, C)))
    ROUNDS, FLUSH_AFTER = 8, 3

    def one_round(outs):
        dW, db, dWd = fenced(K * N), fenced(N), fenced(k * k * C)
        dA = dZ.clone()
        rcs = (L.mkws_op_gemm(ops.p(X), ops.p(dZ), ops.p(dW.mid), K, N, M, K, N, N, 1, 0, 0, ks, ops.s()),
               L.mkws_op_bias_act_bwd(ops.p(Zb), ops.p(bias), 1, ops.p(dA), ops.p(db.mid), M, N, ops.s()),
               L.mkws_op_dwconv_bwd(ops.p(Xd), ops.p(Wd), ops.p(dZd), None, ops.p(dWd.mid), B, H, W, C, k, 1, 1, 1, H, W, ops.s()))
        outs += [dW, db, dWd]
        return rcs

    # the needs, read from the refusals as in (a)
    ops.check(L.mkws_op_set_scratch(None, 0))
    needs = []
    dW, db, dWd, dA = fenced(K * N), fenced(N), fenced(k * k * C), dZ.clone()
    for call in (lambda: L.mkws_op_gemm(ops.p(X), ops.p(dZ), ops.p(dW.mid), K, N, M, K, N, N, 1, 0, 0, ks, ops.s()),
                 lambda: L.mkws_op_bias_act_bwd(ops.p(Zb), ops.p(bias), 1, ops.p(dA), ops.p(db.mid), M, N, ops.s()),
                 lambda: L.mkws_op_dwconv_bwd(ops.p(Xd), ops.p(Wd), ops.p(dZd), None, ops.p(dWd.mid), B, H, W, C, k, 1, 1, 1, H, W, ops.s())):
        assert call() == INVALID_ARG
        needs.append(int(re.search(r"(\d+) floats", L.mkws_last_error().decode()).group(1)))
    ops.check(L.mkws_op_set_scratch(ops.p(ops.scratch), ops.scratch.numel()))
    assert needs == [ks * K * N, min(_ceil(M, 64), 64) * N, dw_bwd_chunks(B * H * W, C) * k * k * C]
    per_round = sum(_r64(n) for n in needs)                          # fold_defer advances the bump pointer by each need rounded up to 64 floats
    queued = per_round * max(FLUSH_AFTER + 1, ROUNDS - FLUSH_AFTER - 1)  # between two explicit flushes
    assert 3 * (FLUSH_AFTER + 1) <= 24                               # the 24-entry queue never fills: only the arena can force a flush here

    def run(defer):
        outs = []
        ops.check(L.mkws_op_fold_defer(1 if defer else 0, ops.s()))
        for r in range(ROUNDS):
            rcs = one_round(outs)
            assert rcs == (0, 0, 0), (r, rcs, L.mkws_last_error())
            if defer and r == FLUSH_AFTER:
                ops.check(L.mkws_op_fold_flush(ops.s()))
        ops.check(L.mkws_op_fold_defer(0, ops.s()))
        torch.cuda.synchronize()
        return outs

    ref = run(False)
    assert all(bool(torch.isfinite(f.mid).all()) for f in ref)
    mid_round = per_round * 5 // 2
    assert mid_round % per_round != 0 and max(needs) < mid_round < queued and max(needs) < queued      # the two tight arenas must flush ...
    assert queued <= ops.scratch.numel()                                                              # ... and the control never has to
    for floats in (mid_round, max(needs)):
        with bound_arena(ops, floats) as arena:
            got = run(True)
            assert arena.pads_intact(), floats
            for n, (g, r) in enumerate(zip(got, ref)):
                assert g.pads_intact() and torch.equal(_bits(g.mid), _bits(r.mid)), (floats, n)
    ops.scratch.fill_(float("nan"))                                  # the control: the module's big arena, NaN-filled like the others
    got = run(True)
    for n, (g, r) in enumerate(zip(got, ref)):
        assert g.pads_intact() and torch.equal(_bits(g.mid), _bits(r.mid)), ("big arena", n)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# (d) one whole step of each trainer
def test_dscnn_step_in_a_fenced_arena():
    from multilingual_kws_amd import dscnn_trainer
    from tests import dscnn_train_cases as cases
    B = 3
    x, y = cases.clips(100)[:B], cases.labels_for(B)
    arena = fenced(4 << 20)                                          # the default size
    runs = []
    for scratch in (None, arena.mid):
        tr = dscnn_trainer.DSCNNTrainer(cases.params(), max_batch=B, seed=5, weight_decay=1e-4, scratch=scratch)
        stats = tr.forward_backward(x, y).clone()
        grads = tr.grads.clone()
        batch = tr.batch_statistics()
        tr.adam_step(5e-4)
        torch.cuda.synchronize()
        runs.append((stats, grads, batch, tr.params_dev.clone(), tr.m.clone(), tr.v.clone()))
    assert tr._scratch.data_ptr() == arena.mid.data_ptr() and tr._scratch.numel() == 4 << 20
    assert arena.pads_intact()
    (s0, g0, b0, p0, m0, v0), (s1, g1, b1, p1, m1, v1) = runs
    for name, a, b in (("loss / correct", s0, s1), ("gradients", g0, g1), ("parameters", p0, p1), ("Adam m", m0, m1), ("Adam v", v0, v1)):
        assert bool(torch.isfinite(b).all()) and torch.equal(_bits(a), _bits(b)), name
    assert bool(g1.any())
    assert b0.keys() == b1.keys() and len(b0) > 0
    for prefix in b0:
        for u, w in zip(b0[prefix], b1[prefix]):
            assert np.array_equal(np.asarray(u), np.asarray(w)) and np.isfinite(np.asarray(w)).all(), prefix


def test_embedding_step_in_fenced_arenas():
    """forward_train and backward at the batch of test_training_mode_gradients_match_the_oracle (tests/test_train_gpu.py), the arenas of both
    streams fenced and NaN-filled, against a twin on default arenas"""
    from multilingual_kws_amd import weights
    from multilingual_kws_amd.embedding_trainer import EmbeddingTrainer
    blob = weights.synthetic_blob()
    rng = np.random.default_rng(3)
    B = 6
    spec = torch.from_numpy(rng.integers(0, 670, size=(B, 49, 40)).astype(np.float32) * np.float32(10 / 256)).cuda()
    d_emb = torch.from_numpy(np.tile(rng.standard_normal(1024).astype(np.float32), (B, 1))).cuda()
    masks = {"2b": np.array([1, 1, 0, 1, 1, 1], bool), "4c": np.array([1, 0, 1, 1, 0, 1], bool), "6d": np.array([0, 1, 1, 1, 1, 1], bool)}
    main, side = fenced(16 << 20), fenced(16 << 20)                  # the default sizes
    runs = []
    for kw in ({}, {"scratch": main.mid, "scratch_side": side.mid}):
        tr = EmbeddingTrainer(blob, **kw)
        emb = tr.forward_train(spec, masks).clone()
        tr.backward(d_emb)
        torch.cuda.synchronize()
        runs.append((emb, tr.grads.clone(), tr.params.clone()))
    assert tr._scratch.data_ptr() == main.mid.data_ptr()
    if tr._side is not None:                                         # the weight-gradient stream ran (MKWS_TRAIN_WGRAD_STREAM): in the caller's arena
        assert tr._scratch_side.data_ptr() == side.mid.data_ptr()
    assert main.pads_intact() and side.pads_intact()
    for name, a, b in zip(("embedding", "gradients", "parameters and moving statistics"), runs[0], runs[1]):
        assert bool(torch.isfinite(b).all()) and torch.equal(_bits(a), _bits(b)), name
    assert bool(runs[1][1].any())
