"""-m gpu: the training operators (mkws_op_*) at the row counts where their launchers change kernel, chunk count or grid.  Every case is ONE
operator call through the C-ABI against a float64 numpy / torch-CPU reference of the same mathematics (float64 autograd or closed form, never
another kernel).  The shapes are functions of the launch constants the library reports (mkws_op_get_option: "bn_small_rows", "bn_chunk_cap",
"bn_apply_chunk_cap", "bn_max_chunks", "bn_max_gemm_tiles", "grid_cap"), and every case asserts up front that its shape lies on the intended side
of the constant: a retune moves the cases with it.  Bounds: the ones tests/test_train_gpu.py holds each operator to."""
import types

import numpy as np
import pytest

from tests.util_train_ops import make_ops

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
F = torch.nn.functional
EPS = 1e-3


def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-30))


def _np(t):
    return t.detach().cpu().numpy()


def _ceil(a, b):
    return (a + b - 1) // b


@pytest.fixture(scope="module")
def ops():
    return make_ops()


@pytest.fixture(scope="module")
def c(ops):
    k = types.SimpleNamespace()
    for name in ("bn_small_rows", "bn_chunk_cap", "bn_apply_chunk_cap", "bn_max_chunks", "bn_max_gemm_tiles", "grid_cap"):
        v = ops.L.mkws_op_get_option(name.encode())
        assert v > 0, name
        setattr(k, name, v)
    return k


@pytest.fixture(autouse=True)
def _arena(ops):
    ops.check(ops.L.mkws_op_set_scratch(ops.p(ops.scratch), ops.scratch.numel()))


def _new(ops, *shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device=ops.dev)


def _channels(rng, M, C, offset=1.0, lo=0.2, hi=3.0):
    """[M, C] float32 with a scale and an offset of its own per channel"""
    return (rng.standard_normal((M, C)) * rng.uniform(lo, hi, C) + offset * rng.standard_normal(C)).astype(np.float32)


def _act64(y, act):
    return y * torch.sigmoid(y) if act == 1 else y


# ---------------------------------------------------------------------------------------------------------------------------------------------
# BatchNorm forward: statistics, fused training forward, normalise
BN_ROWS = {
    "last-uncapped": lambda c: c.bn_chunk_cap * 128,             # bn_chunk_cap chunks of exactly 128 rows: the last M before the cap binds
    "cap+1": lambda c: c.bn_chunk_cap * 128 + 1,                 # the cap binds: chunks of ceil(M / cap) = 129 rows, the last one nearly empty
    "cap+129": lambda c: c.bn_chunk_cap * 128 + 129,             # the cap binds, uneven last chunk
    "apply-cap+200": lambda c: c.bn_apply_chunk_cap * 128 + 200,  # the normalise / apply launches' cap binds as well
}


def _assert_bn_route(c, rows, M):
    chunks, apply_chunks = min(_ceil(M, 128), c.bn_chunk_cap), min(_ceil(M, 128), c.bn_apply_chunk_cap)
    per = _ceil(M, chunks)
    if rows == "last-uncapped":
        assert _ceil(M, 128) == c.bn_chunk_cap and per == 128 and _ceil(M + 1, 128) > c.bn_chunk_cap
    else:
        assert _ceil(M, 128) > c.bn_chunk_cap and per > 128
    if rows == "cap+129":
        assert M % per != 0                                       # uneven last chunk
    if rows == "apply-cap+200":
        assert _ceil(M, 128) > c.bn_apply_chunk_cap and _ceil(M, apply_chunks) > 128
    else:
        assert _ceil(M, 128) <= c.bn_apply_chunk_cap
    return chunks, apply_chunks


def _bn_forward_check(ops, Z, gamma, beta, act, res=None, keep=None, group=1, repeat=True):
    """mkws_op_bn_stats, mkws_op_bn_train_fwd_res and mkws_op_bn_act_fwd on Z against float64: mean, biased variance, moving statistics
    (momentum 0.99 from zeros / ones, variance Bessel-corrected) and the output."""
    M, C = Z.shape
    z = Z.astype(np.float64)
    mean, var = z.mean(0), z.var(0)
    y = torch.from_numpy(gamma.astype(np.float64) * (z - mean) / np.sqrt(var + EPS) + beta.astype(np.float64))
    a = _act64(y, act).numpy()
    out = a if res is None else a * (keep.astype(np.float64)[np.arange(M) // group][:, None] if keep is not None else 1.0) + res.astype(np.float64)
    bessel = M / max(M - 1, 1)
    dZ, dg, db = ops.t(Z), ops.t(gamma), ops.t(beta)
    dm, dv = _new(ops, C), _new(ops, C)
    ops.check(ops.L.mkws_op_bn_stats(ops.p(dZ), M, C, ops.p(dm), ops.p(dv), ops.s()))
    errs = {"stats mean": _rel(_np(dm), mean), "stats var": _rel(_np(dv), var) if var.max() > 0 else float(np.abs(_np(dv)).max())}
    A0 = _new(ops, M, C)
    ops.check(ops.L.mkws_op_bn_act_fwd(ops.p(dZ), ops.p(dm), ops.p(dv), ops.p(dg), ops.p(db), EPS, act, ops.p(A0), M, C, ops.s()))
    errs["bn_act_fwd"] = _rel(_np(A0), a)
    dR, dK = (ops.t(res) if res is not None else None), (ops.t(keep) if keep is not None else None)
    outs = []
    for _ in range(2 if repeat else 1):
        mm, mv, m2, v2, A = ops.t(np.zeros(C)), ops.t(np.ones(C)), _new(ops, C), _new(ops, C), _new(ops, M, C)
        ops.check(ops.L.mkws_op_bn_train_fwd_res(ops.p(dZ), M, C, ops.p(dg), ops.p(db), EPS, act, 0.99, ops.p(mm), ops.p(mv), ops.p(m2), ops.p(v2), ops.p(A),
                                                 ops.p(dR), ops.p(dK), group, ops.s()))
        outs.append((mm, mv, m2, v2, A))
    mm, mv, m2, v2, A = outs[0]
    errs.update({"mean": _rel(_np(m2), mean), "var": _rel(_np(v2), var) if var.max() > 0 else float(np.abs(_np(v2)).max()),
                 "moving mean": _rel(_np(mm), 0.01 * mean), "moving var": _rel(_np(mv), 0.99 + 0.01 * var * bessel), "out": _rel(_np(A), out)})
    print(f"bn forward M={M} C={C}:", {k: f"{v:.2e}" for k, v in errs.items()})
    if repeat:                                                    # fixed-order chunk folds: a second call returns the same bits
        assert all(torch.equal(p, q) for p, q in zip(outs[0], outs[1]))
    assert torch.equal(m2, dm) and torch.equal(v2, dv)            # the statistics launch and the fused forward fold the same chunks in the same order
    return errs


def _quad_lanes(C):
    """bn_lanes: quad lanes of each 64-channel slab of a [M, C] launch -- 4, 8 or 16 by the slab's live channel quads"""
    live = [(min(C - s, 64) + 3) // 4 for s in range(0, C, 64)]
    return [16 if q > 8 else (8 if q > 4 else 4) for q in live]


# C = 16: 4 quad lanes (64 row lanes); 24: 8 quad lanes, two of them idle; 40: 16 quad lanes, six idle; 100: a full slab and one with 9 live quads
BN_WIDTHS = [16, 24, 40, 100]


def test_batchnorm_widths_cover_the_lane_layouts():
    assert [_quad_lanes(C) for C in BN_WIDTHS] == [[4], [8], [16], [16, 16]] and (100 - 64) // 4 == 9


@pytest.mark.parametrize("C", BN_WIDTHS)
@pytest.mark.parametrize("rows", list(BN_ROWS))
def test_batchnorm_forward_at_the_chunk_caps(ops, c, rows, C):
    M = BN_ROWS[rows](c)
    _assert_bn_route(c, rows, M)
    rng = np.random.default_rng(M + C)
    Z = _channels(rng, M, C)
    gamma, beta = rng.uniform(0.5, 1.5, C).astype(np.float32), (0.1 * rng.standard_normal(C)).astype(np.float32)
    errs = _bn_forward_check(ops, Z, gamma, beta, act=0 if C == 40 else 1)
    assert max(errs.values()) < 1e-5, errs


def test_batchnorm_forward_residual_groups_straddle_chunks(ops, c):
    """out = keep[row // 35] * BN(Z) + shortcut with the chunk cap binding: neither the statistics chunks nor the normalise chunks hold whole groups."""
    M, C, group = BN_ROWS["cap+129"](c), 40, 35
    chunks, apply_chunks = _assert_bn_route(c, "cap+129", M)
    assert _ceil(M, chunks) % group != 0 and _ceil(M, apply_chunks) % group != 0
    rng = np.random.default_rng(7)
    Z, res = _channels(rng, M, C), _channels(rng, M, C)
    keep = ((rng.random(_ceil(M, group)) > 0.3) / 0.7).astype(np.float32)
    gamma, beta = rng.uniform(0.5, 1.5, C).astype(np.float32), (0.1 * rng.standard_normal(C)).astype(np.float32)
    errs = _bn_forward_check(ops, Z, gamma, beta, act=1, res=res, keep=keep, group=group)
    assert max(errs.values()) < 1e-5, errs


def test_batchnorm_statistics_do_not_cancel(ops, c):
    """Per-channel offset 50, standard deviation 0.1, capped chunks: E[z^2] - E[z]^2 in float32 would lose the variance (0.01 against 2500)."""
    M, C = BN_ROWS["cap+129"](c), 16
    _assert_bn_route(c, "cap+129", M)
    rng = np.random.default_rng(50)
    Z = (50.0 + 0.1 * rng.standard_normal((M, C))).astype(np.float32)
    gamma, beta = rng.uniform(0.5, 1.5, C).astype(np.float32), (0.1 * rng.standard_normal(C)).astype(np.float32)
    naive = (Z.astype(np.float32) ** 2).mean(0, dtype=np.float32) - Z.mean(0, dtype=np.float32) ** 2
    assert _rel(naive, Z.astype(np.float64).var(0)) > 1e-3        # the input does tell the two formulas apart
    errs = _bn_forward_check(ops, Z, gamma, beta, act=1)
    assert max(errs.values()) < 1e-5, errs


@pytest.mark.parametrize("M", [1, 2])
def test_batchnorm_forward_one_and_two_rows(ops, c, M):
    """One chunk with one or two rows: variance 0 / (a - b)^2 / 4; the moving variance takes the factor M / max(M - 1, 1)."""
    C = 8
    assert M <= 128 <= c.bn_chunk_cap * 128
    rng = np.random.default_rng(M)
    Z = _channels(rng, M, C)
    gamma, beta = rng.uniform(0.5, 1.5, C).astype(np.float32), (0.1 * rng.standard_normal(C)).astype(np.float32)
    errs = _bn_forward_check(ops, Z, gamma, beta, act=1)
    if M == 1:
        assert errs["var"] == 0.0 and errs["stats var"] == 0.0
    assert max(errs.values()) < 1e-5, errs


# ---------------------------------------------------------------------------------------------------------------------------------------------
# BatchNorm backward with the gradient assembly, small and large routes
BWD_ROWS = dict({"4": lambda c: 4, "100": lambda c: 100, "127": lambda c: 127, "129": lambda c: 129,
                 "small-last": lambda c: c.bn_small_rows,        # the last M of the one-launch kernel
                 "small+1": lambda c: c.bn_small_rows + 1},      # the first M of the two-launch form
                **{k: BN_ROWS[k] for k in ("cap+129", "apply-cap+200")})
FORMS = {"src": (1, 0, 0), "src*row_scale": (1, 1, 0), "bcast": (0, 0, 1), "src*row_scale+bcast": (1, 1, 1)}


@pytest.mark.parametrize("C", BN_WIDTHS)
@pytest.mark.parametrize("rows", list(BWD_ROWS))
def test_batchnorm_backward_with_gradient_assembly(ops, c, rows, C):
    """mkws_op_bn_act_bwd_ex against float64 autograd of act(BN(z)) under the incoming gradient dA = src * keep[row // group] + bcast[row // group]
    * bscale: dZ, dgamma, dbeta, for act 0 / 1 and the four argument forms; src stays intact."""
    M = BWD_ROWS[rows](c)
    if rows in ("4", "100", "127", "129", "small-last"):
        assert M <= c.bn_small_rows                               # bn_small_bwd_kernel: one launch, 128 row lanes (M = 4, 100, 127: idle lanes; 129: a second row)
    elif rows == "small+1":
        assert c.bn_small_rows < M <= c.bn_chunk_cap * 128        # bn_act_bwd_reduce_kernel + bn_bwd_apply_kernel, chunks of 128 rows
    else:
        assert M > c.bn_small_rows
        _assert_bn_route(c, rows, M)                              # the two launches with their chunk caps binding
    group = 35 if M > 35 else 3
    nb = _ceil(M, group)
    rng = np.random.default_rng(3 * M + C)
    Z = _channels(rng, M, C)
    gamma, beta = rng.uniform(0.5, 1.5, C).astype(np.float32), (0.1 * rng.standard_normal(C)).astype(np.float32)
    S, bc = rng.standard_normal((M, C)).astype(np.float32), rng.standard_normal((nb, C)).astype(np.float32)
    keep = ((rng.random(nb) > 0.3) / 0.7).astype(np.float32)
    keep[0], keep[-1] = 0.0, 1.0 / 0.7                            # (both values occur, also with two groups)
    bscale = 1.0 / group
    z64 = torch.tensor(Z, dtype=torch.float64)
    mean, var = z64.mean(0), z64.var(0, unbiased=False)
    dZ, dg, db, dmean, dvar = ops.t(Z), ops.t(gamma), ops.t(beta), ops.t(mean.numpy()), ops.t(var.numpy())
    dS, dK, dB = ops.t(S), ops.t(keep), ops.t(bc)
    S_before = dS.clone()
    row_group = np.arange(M) // group
    worst = {}
    for act in (0, 1):
        for form, (has_src, has_rs, has_bc) in FORMS.items():
            dA = np.zeros((M, C))
            if has_src:
                dA = S.astype(np.float64) * (keep.astype(np.float64)[row_group][:, None] if has_rs else 1.0)
            if has_bc:
                dA = dA + bc.astype(np.float64)[row_group] * np.float64(np.float32(bscale))
            z = z64.clone().requires_grad_(True)
            g, b = torch.tensor(gamma, dtype=torch.float64, requires_grad=True), torch.tensor(beta, dtype=torch.float64, requires_grad=True)
            y = g * (z - z.mean(0)) / torch.sqrt(z.var(0, unbiased=False) + EPS) + b
            (_act64(y, act) * torch.from_numpy(dA)).sum().backward()
            outs = []
            for _ in range(2 if form == "src*row_scale+bcast" else 1):
                d, gg, gb = _new(ops, M, C), _new(ops, C), _new(ops, C)
                ops.check(ops.L.mkws_op_bn_act_bwd_ex(ops.p(dZ), ops.p(dmean), ops.p(dvar), ops.p(dg), ops.p(db), EPS, act, ops.p(d), ops.p(dS) if has_src else None,
                                                      ops.p(dK) if has_rs else None, ops.p(dB) if has_bc else None, bscale, group, ops.p(gg), ops.p(gb), M, C, ops.s()))
                outs.append((d, gg, gb))
            d, gg, gb = outs[0]
            errs = (_rel(_np(d), z.grad.numpy()), _rel(_np(gg), g.grad.numpy()), _rel(_np(gb), b.grad.numpy()))
            worst[(act, form)] = max(errs)
            assert max(errs) < 2e-4, (act, form, errs)
            if len(outs) == 2:                                     # chunk sums fold in a fixed order: the same bits again
                assert all(torch.equal(p, q) for p, q in zip(outs[0], outs[1])), (act, form)
    assert torch.equal(dS, S_before)                              # the source gradient stays intact (the shortcut still needs it)
    print(f"bn backward M={M} C={C}: worst relative error {max(worst.values()):.2e}")


# ---------------------------------------------------------------------------------------------------------------------------------------------
# depthwise weight / input gradient with the chunk cap binding
@pytest.mark.parametrize("H,W,C,k,s,B,cap", [(7, 5, 240, 5, 1, 120, 128),      # 4 quad slabs, 4 200 positions
                                             (4, 3, 672, 5, 2, 400, 47),       # 11 slabs, 1 600 positions
                                             (2, 2, 1152, 3, 1, 300, 29),      # 18 slabs, 1 200 positions; 29 chunks of 10 368 sums: the 4-sub-lane fold
                                             (13, 10, 144, 5, 2, 260, 171)])   # 3 slabs, 9 100 positions
def test_depthwise_backward_with_capped_chunks(ops, H, W, C, k, s, B, cap):
    """mkws_op_dwconv_bwd once min(ceil(512 / slabs), 256) caps the position chunks: a chunk is ceil(npos / chunks) positions, its boundaries fall
    inside clips and image rows, and 16 position lanes stride it.  dX, dW against float64 conv2d autograd; also with dX = NULL and with dW = NULL."""
    from oracle.efficientnet_oracle import correct_pad
    rng = np.random.default_rng(H * C + B)
    X = _channels(rng, B * H * W, C, lo=0.5, hi=1.5, offset=0.3).reshape(B, H, W, C)
    Wt = rng.standard_normal((k, k, C)).astype(np.float32)
    if s == 2:
        (pt, pb), (pl, pr) = correct_pad(H, W, k)
    else:
        pt = pb = pl = pr = k // 2
    x = torch.tensor(X, dtype=torch.float64).permute(0, 3, 1, 2).requires_grad_(True)
    w = torch.tensor(Wt, dtype=torch.float64).permute(2, 0, 1)[:, None].requires_grad_(True)
    z = F.conv2d(F.pad(x, (pl, pr, pt, pb)), w, stride=s, groups=C)
    Ho, Wo = z.shape[2], z.shape[3]
    npos, xb = B * Ho * Wo, _ceil(C // 4, 16)
    assert cap == min(_ceil(512, xb), 256) and _ceil(npos, 32) > cap         # the cap binds ...
    assert _ceil(npos, cap) % (Ho * Wo) != 0 and npos % cap != 0             # ... chunks end inside clips, and the last chunk is short
    dZ = rng.standard_normal((B, Ho, Wo, C)).astype(np.float32)
    (z * torch.tensor(dZ, dtype=torch.float64).permute(0, 3, 1, 2)).sum().backward()
    dX_ref, dW_ref = x.grad.permute(0, 2, 3, 1).numpy(), w.grad[:, 0].permute(1, 2, 0).numpy()
    dx, dw, dz = ops.t(X), ops.t(Wt), ops.t(dZ)
    call = lambda gX, gW: ops.check(ops.L.mkws_op_dwconv_bwd(ops.p(dx), ops.p(dw), ops.p(dz), ops.p(gX), ops.p(gW), B, H, W, C, k, s, pt, pl, Ho, Wo, ops.s()))
    gX, gW = _new(ops, B, H, W, C), _new(ops, k, k, C)
    call(gX, gW)
    errs = (_rel(_np(gX), dX_ref), _rel(_np(gW), dW_ref))
    print(f"depthwise backward {(H, W, C, k, s, B)}: dX {errs[0]:.2e} dW {errs[1]:.2e}")
    assert errs[0] < 1e-5 and errs[1] < 1e-4, errs
    gW2, gX2 = _new(ops, k, k, C), _new(ops, B, H, W, C)
    call(None, gW2)                                               # the weight gradient alone (the trainer's second stream): same bits, fixed-order fold
    call(gX2, None)                                               # the input gradient alone
    assert torch.equal(gW2, gW) and torch.equal(gX2, gX)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# stem
@pytest.mark.parametrize("B", [132, 140])
def test_stem_forward_and_weight_gradient_with_capped_workgroups(ops, B):
    """mkws_op_stem_bwd_weight once min(ceil(B * 500 / 256), 256) workgroups cap (from 132 clips): a workgroup's pixels are ceil(B * 500 / 256),
    no multiple of the 32 pixel lanes; the 256 partial slabs of 288 sums take the 16-sub-lane fold."""
    assert _ceil(B * 500, 256) > 256 and _ceil(131 * 500, 256) <= 256 and _ceil(B * 500, 256) % 32 != 0
    rng = np.random.default_rng(B)
    spec = (rng.integers(0, 670, size=(B, 49, 40)) * (10 / 256)).astype(np.float32)
    Wt = rng.standard_normal((3, 3, 1, 32)).astype(np.float32)
    x = (torch.tensor(spec, dtype=torch.float64)[:, None] / 255.0 - 0.1) / 0.7
    w = torch.tensor(Wt, dtype=torch.float64).permute(3, 2, 0, 1).requires_grad_(True)
    z = F.conv2d(F.pad(x, (0, 1, 1, 1)), w, stride=2)
    dZ = _channels(rng, B * 500, 32, lo=0.5, hi=1.5, offset=0.3).reshape(B, 25, 20, 32)
    (z * torch.tensor(dZ, dtype=torch.float64).permute(0, 3, 1, 2)).sum().backward()
    ds, dw, Z = ops.t(spec), ops.t(Wt), _new(ops, B, 25, 20, 32)
    ops.check(ops.L.mkws_op_stem_fwd(ops.p(ds), ops.p(dw), 0.1, 0.7, ops.p(Z), B, ops.s()))
    assert _rel(_np(Z), z.detach().permute(0, 2, 3, 1).numpy()) < 1e-5
    ddZ, gW, gW2 = ops.t(dZ), _new(ops, 3, 3, 1, 32), _new(ops, 3, 3, 1, 32)
    ops.check(ops.L.mkws_op_stem_bwd_weight(ops.p(ds), ops.p(ddZ), 0.1, 0.7, ops.p(gW), B, ops.s()))
    ops.check(ops.L.mkws_op_stem_bwd_weight(ops.p(ds), ops.p(ddZ), 0.1, 0.7, ops.p(gW2), B, ops.s()))
    err = _rel(_np(gW), w.grad.permute(2, 3, 1, 0).numpy())
    print(f"stem dW B={B}: {err:.2e}")
    assert err < 1e-4 and torch.equal(gW2, gW)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# bias + activation backward
@pytest.mark.parametrize("M,N,capped", [(4097, 50, True),        # 65 chunks of 64 rows wanted, 64 given: chunks of 65 rows, the last one 2
                                        (8200, 72, True),        # chunks of 129 rows, two channel slabs
                                        (4096, 4, False)])       # the last M with chunks of 64 rows; one quad of channels
def test_bias_activation_backward_with_capped_chunks(ops, M, N, capped):
    """mkws_op_bias_act_bwd: min(ceil(M / 64), 64) row chunks (64 partial rows: the 16-sub-lane fold), activations 1-4, dA and dbias."""
    assert (_ceil(M, 64) > 64) == capped and _ceil(M, 64) >= 64
    rng = np.random.default_rng(M + N)
    Zb, bias, dAb = _channels(rng, M, N, lo=0.5, hi=1.5, offset=0.5), rng.standard_normal(N).astype(np.float32), _channels(rng, M, N, lo=0.5, hi=1.5, offset=0.3)
    fns = {1: lambda y: y * torch.sigmoid(y), 2: torch.relu, 3: torch.selu, 4: torch.sigmoid}
    dZb, dbias = ops.t(Zb), ops.t(bias)
    for act, fn in fns.items():
        zz, bb = torch.tensor(Zb, dtype=torch.float64, requires_grad=True), torch.tensor(bias, dtype=torch.float64, requires_grad=True)
        (fn(zz + bb) * torch.tensor(dAb, dtype=torch.float64)).sum().backward()
        d, gb, d2, gb2 = ops.t(dAb), _new(ops, N), ops.t(dAb), _new(ops, N)
        ops.check(ops.L.mkws_op_bias_act_bwd(ops.p(dZb), ops.p(dbias), act, ops.p(d), ops.p(gb), M, N, ops.s()))
        ops.check(ops.L.mkws_op_bias_act_bwd(ops.p(dZb), ops.p(dbias), act, ops.p(d2), ops.p(gb2), M, N, ops.s()))
        errs = (_rel(_np(d), zz.grad.numpy()), _rel(_np(gb), bb.grad.numpy()))
        print(f"bias backward {(M, N)} act {act}: dA {errs[0]:.2e} dbias {errs[1]:.2e}")
        assert max(errs) < 1e-5, (act, errs)
        assert torch.equal(d2, d) and torch.equal(gb2, gb), act


# ---------------------------------------------------------------------------------------------------------------------------------------------
# depthwise conv + BN and conv + BN at the edge between fused statistics and the three-launch sequence
@pytest.mark.parametrize("side", ["fused-last", "sequence-first"])
def test_depthwise_batchnorm_at_the_fusion_edge(ops, c, side):
    """mkws_op_dwconv_bn_fwd with exactly bn_max_chunks chunks of 128 output rows (the convolution leaves the chunk statistics) and one clip more
    (convolution, statistics, normalise: three launches): convolution, statistics, moving statistics and output against float64."""
    H = W = 2
    k, s, C = 3, 1, 8
    assert (c.bn_max_chunks * 128) % (H * W) == 0
    B = c.bn_max_chunks * 128 // (H * W) + (side == "sequence-first")
    M = B * H * W
    if side == "fused-last":
        assert _ceil(M, 128) == c.bn_max_chunks and _ceil(M + H * W, 128) > c.bn_max_chunks      # one clip more would leave the fused route
    else:
        assert _ceil(M, 128) > c.bn_max_chunks and _ceil(M - H * W, 128) <= c.bn_max_chunks       # the first B of the three-launch sequence
    rng = np.random.default_rng(B)
    X = _channels(rng, M, C, lo=0.5, hi=2.0).reshape(B, H, W, C)
    Wd = (rng.standard_normal((k, k, C)) / k).astype(np.float32)
    gamma, beta = rng.uniform(0.5, 1.5, C).astype(np.float32), (0.1 * rng.standard_normal(C)).astype(np.float32)
    x, w = torch.tensor(X, dtype=torch.float64).permute(0, 3, 1, 2), torch.tensor(Wd, dtype=torch.float64).permute(2, 0, 1)[:, None]
    z = F.conv2d(F.pad(x, (1, 1, 1, 1)), w, groups=C).permute(0, 2, 3, 1).reshape(M, C).numpy()
    mean, var = z.mean(0), z.var(0)
    a = _act64(torch.from_numpy(gamma * (z - mean) / np.sqrt(var + EPS) + beta), 1).numpy()
    dX, dW, dg, db = ops.t(X), ops.t(Wd), ops.t(gamma), ops.t(beta)
    outs = []
    for _ in range(2):
        mm, mv = ops.t(np.zeros(C)), ops.t(np.ones(C))
        Z, m1, v1, A = _new(ops, M, C), _new(ops, C), _new(ops, C), _new(ops, M, C)
        ops.check(ops.L.mkws_op_dwconv_bn_fwd(ops.p(dX), ops.p(dW), ops.p(Z), B, H, W, C, k, s, 1, 1, H, W, ops.p(dg), ops.p(db), EPS, 1, 0.99, ops.p(mm), ops.p(mv),
                                              ops.p(m1), ops.p(v1), ops.p(A), ops.s()))
        outs.append((Z, m1, v1, A, mm, mv))
    Z, m1, v1, A, mm, mv = outs[0]
    errs = {"Z": _rel(_np(Z), z), "mean": _rel(_np(m1), mean), "var": _rel(_np(v1), var), "moving mean": _rel(_np(mm), 0.01 * mean),
            "moving var": _rel(_np(mv), 0.99 + 0.01 * var * M / (M - 1)), "out": _rel(_np(A), a)}
    print(f"depthwise + BN {side} M={M}:", {k_: f"{v:.2e}" for k_, v in errs.items()})
    assert max(errs.values()) < 1e-5, errs
    assert all(torch.equal(p, q) for p, q in zip(outs[0], outs[1]))


@pytest.mark.parametrize("side,res", [("fused-last", False), ("sequence-first", True)])
def test_conv_batchnorm_at_the_fusion_edge(ops, c, side, res):
    """mkws_op_conv_bn_fwd with exactly bn_max_gemm_tiles 64-row tiles (statistics in the GEMM epilogue, one chunk per tile) and one row more (the
    three-launch sequence; this case with the residual branch, keep[row // 35]): product, statistics, moving statistics and output against float64."""
    K, N, group = 16, 24, 35
    M = c.bn_max_gemm_tiles * 64 + (side == "sequence-first")
    assert (_ceil(M, 64) <= c.bn_max_gemm_tiles) == (side == "fused-last") and _ceil(c.bn_max_gemm_tiles * 64 + 1, 64) > c.bn_max_gemm_tiles
    rng = np.random.default_rng(M)
    X, Wt = _channels(rng, M, K, lo=0.5, hi=1.5, offset=0.3), (rng.standard_normal((K, N)) / np.sqrt(K)).astype(np.float32)
    gamma, beta = rng.uniform(0.5, 1.5, N).astype(np.float32), (0.1 * rng.standard_normal(N)).astype(np.float32)
    R = _channels(rng, M, N) if res else None
    keep = ((rng.random(_ceil(M, group)) > 0.3) / 0.7).astype(np.float32) if res else None
    z = X.astype(np.float64) @ Wt.astype(np.float64)
    mean, var = z.mean(0), z.var(0)
    a = _act64(torch.from_numpy(gamma * (z - mean) / np.sqrt(var + EPS) + beta), 1).numpy()
    if res:
        a = a * keep.astype(np.float64)[np.arange(M) // group][:, None] + R.astype(np.float64)
    dX, dW, dg, db = ops.t(X), ops.t(Wt), ops.t(gamma), ops.t(beta)
    dR, dK = (ops.t(R), ops.t(keep)) if res else (None, None)
    outs = []
    for _ in range(2):
        mm, mv = ops.t(np.zeros(N)), ops.t(np.ones(N))
        Z, m1, v1, A = _new(ops, M, N), _new(ops, N), _new(ops, N), _new(ops, M, N)
        ops.check(ops.L.mkws_op_conv_bn_fwd(ops.p(dX), ops.p(dW), ops.p(Z), M, N, K, ops.p(dg), ops.p(db), EPS, 1, 0.99, ops.p(mm), ops.p(mv), ops.p(m1), ops.p(v1),
                                            ops.p(A), ops.p(dR), ops.p(dK), group, ops.s()))
        outs.append((Z, m1, v1, A, mm, mv))
    Z, m1, v1, A, mm, mv = outs[0]
    errs = {"Z": _rel(_np(Z), z), "mean": _rel(_np(m1), mean), "var": _rel(_np(v1), var), "moving mean": _rel(_np(mm), 0.01 * mean),
            "moving var": _rel(_np(mv), 0.99 + 0.01 * var * M / (M - 1)), "out": _rel(_np(A), a)}
    print(f"conv + BN {side} M={M}:", {k_: f"{v:.2e}" for k_, v in errs.items()})
    assert max(errs.values()) < 1e-5, errs
    assert all(torch.equal(p, q) for p, q in zip(outs[0], outs[1]))


# ---------------------------------------------------------------------------------------------------------------------------------------------
# grid-stride loops: one element count for all, grid_cap * 256 + 1003 -- the first 1 003 threads of the capped grid walk a second element
def _grid_n(c):
    n = c.grid_cap * 256 + 1003
    assert _ceil(n, 256) > c.grid_cap and n - c.grid_cap * 256 < 256 * c.grid_cap
    return n


def _split(n):
    """n = rows * cols with the smallest cols in 3..64 that divides n (n itself as one column otherwise)"""
    for d in range(3, 65):
        if n % d == 0:
            return n // d, d
    return n, 1


def test_adam_walks_the_whole_blob(ops, c):
    """mkws_op_adam, three steps against the Keras Adam oracle, and mkws_op_adam_dev (step index on the device) on the same trajectory."""
    from oracle import head_oracle as ho
    n = _grid_n(c)
    rng = np.random.default_rng(n)
    p0, gr = rng.standard_normal(n).astype(np.float32), rng.standard_normal(n).astype(np.float32)
    assert np.abs(p0).max() < 7.9          # float32 spacing below 8 is 4.8e-7: three roundings of a parameter stay under the 1e-6 bound
    P, Gd, m, v = ops.t(p0), ops.t(gr), ops.t(np.zeros(n)), ops.t(np.zeros(n))
    P2, m2, v2, step = ops.t(p0), ops.t(np.zeros(n)), ops.t(np.zeros(n)), torch.zeros(1, dtype=torch.int32, device=ops.dev)
    opt, pr = ho.KerasAdam(n, lr=1e-3), p0.astype(np.float64)
    for t in range(1, 4):
        ops.check(ops.L.mkws_op_adam(ops.p(P), ops.p(Gd), ops.p(m), ops.p(v), n, 1e-3, 0.9, 0.999, 1e-7, t, 0.5, ops.s()))
        ops.check(ops.L.mkws_op_step_inc(ops.p(step), ops.s()))
        ops.check(ops.L.mkws_op_adam_dev(ops.p(P2), ops.p(Gd), ops.p(m2), ops.p(v2), n, 1e-3, 0.9, 0.999, 1e-7, ops.p(step), 0.5, ops.s()))
        pr = opt.step(pr, 0.5 * gr.astype(np.float64))
    got = _np(P)
    err = np.abs(got - pr)
    print(f"adam n={n}: largest error {err.max():.2e}, in the second grid-stride pass {err[c.grid_cap * 256:].max():.2e}")
    assert err.max() < 1e-6
    assert np.abs(got - p0).min() > 0      # every element moved, the tail included
    assert _rel(_np(m), opt.m) < 1e-5 and _rel(_np(v), opt.v) < 1e-4      # (1 - beta2 in float32 is 2e-5 off 0.001)
    assert int(step.item()) == 3 and np.abs(_np(P2) - got).max() < 1e-7


def test_elementwise_operators_beyond_the_grid_cap(ops, c):
    """axpy, bias_act_fwd, bn_act_fwd, row_scale_add, scale_channels and add_bcast over grid_cap * 256 + 1003 elements, every element compared."""
    n = _grid_n(c)
    rng = np.random.default_rng(n + 1)
    M, N = _split(n)
    HW, B = _split(M)                                            # n = B * HW * N
    assert M * N == n and B * HW * N == n
    X, Y = rng.standard_normal(n).astype(np.float32), rng.standard_normal(n).astype(np.float32)
    x64, y64 = X.astype(np.float64), Y.astype(np.float64)
    dXv, dYv = ops.t(X), ops.t(Y)
    tail = slice(c.grid_cap * 256, n)

    def close(got, ref, bound, what):
        got, ref = _np(got).reshape(-1), np.asarray(ref).reshape(-1)
        scale = np.abs(ref).max()
        assert np.abs(got - ref).max() < bound * scale and np.abs(got[tail] - ref[tail]).max() < bound * scale, what
    # y += alpha * x
    y = dYv.clone()
    ops.check(ops.L.mkws_op_axpy(ops.p(y), ops.p(dXv), -2.0, n, ops.s()))
    close(y, y64 - 2.0 * x64, 1e-5, "axpy")
    # A = swish(Z + bias), Z [M, N]
    bias = rng.standard_normal(N).astype(np.float32)
    dbias, A = ops.t(bias), _new(ops, n)
    ops.check(ops.L.mkws_op_bias_act_fwd(ops.p(dXv), ops.p(dbias), 1, ops.p(A), M, N, ops.s()))
    zb = torch.from_numpy(x64.reshape(M, N) + bias.astype(np.float64))
    close(A, (zb * torch.sigmoid(zb)).numpy(), 1e-6, "bias_act_fwd")
    # A = swish(gamma * (Z - mean) * rsqrt(var + eps) + beta)
    mean, var = rng.standard_normal(N).astype(np.float32), rng.uniform(0.5, 2.0, N).astype(np.float32)
    gamma, beta = rng.uniform(0.5, 1.5, N).astype(np.float32), (0.1 * rng.standard_normal(N)).astype(np.float32)
    A = _new(ops, n)
    dm, dv, dg, db = ops.t(mean), ops.t(var), ops.t(gamma), ops.t(beta)
    ops.check(ops.L.mkws_op_bn_act_fwd(ops.p(dXv), ops.p(dm), ops.p(dv), ops.p(dg), ops.p(db), EPS, 1, ops.p(A), M, N, ops.s()))
    yb = torch.from_numpy(gamma.astype(np.float64) * (x64.reshape(M, N) - mean) / np.sqrt(var.astype(np.float64) + np.float64(np.float32(EPS))) + beta)
    close(A, (yb * torch.sigmoid(yb)).numpy(), 1e-5, "bn_act_fwd")
    # out[b, :] = a[b, :] * s[b] + c[b, :], B rows of HW * N
    sc = ((rng.random(B) > 0.3) / 0.7).astype(np.float32)
    dsc, out = ops.t(sc), _new(ops, n)
    ops.check(ops.L.mkws_op_row_scale_add(ops.p(dXv), ops.p(dsc), ops.p(dYv), ops.p(out), B, HW * N, ops.s()))
    close(out, x64.reshape(B, -1) * sc.astype(np.float64)[:, None] + y64.reshape(B, -1), 1e-6, "row_scale_add")
    ops.check(ops.L.mkws_op_row_scale_add(ops.p(dXv), ops.p(dsc), None, ops.p(out), B, HW * N, ops.s()))
    close(out, x64.reshape(B, -1) * sc.astype(np.float64)[:, None], 1e-6, "row_scale_add without c")
    # out[b, hw, c] = A[b, hw, c] * g[b, c];  X[b, hw, c] += v[b, c] * scale
    g = rng.uniform(0, 1, (B, N)).astype(np.float32)
    dgate, out = ops.t(g), _new(ops, n)
    ops.check(ops.L.mkws_op_scale_channels(ops.p(dXv), ops.p(dgate), ops.p(out), B, HW, N, ops.s()))
    close(out, x64.reshape(B, HW, N) * g.astype(np.float64)[:, None], 1e-6, "scale_channels")
    acc = dYv.clone()
    ops.check(ops.L.mkws_op_add_bcast(ops.p(acc), ops.p(dgate), 0.25, B, HW, N, ops.s()))
    close(acc, y64.reshape(B, HW, N) + 0.25 * g.astype(np.float64)[:, None], 1e-6, "add_bcast")


# ---------------------------------------------------------------------------------------------------------------------------------------------
# pooling, SE backward, SE weight gradient
@pytest.mark.parametrize("B,HW,C", [(3, 1, 1280),                # one position: three of the four position lanes stay empty; five quad slabs
                                    (3, 3, 672),                 # three positions: one empty lane; 168 quads = two full slabs and 40 quads
                                    (2, 500, 32),                # the first block's image: 125 positions per lane; 8 live quads of 64
                                    (2, 35, 1152)])              # 35 = 4 * 8 + 3: uneven lanes
def test_pooling_and_se_backward_position_lanes(ops, B, HW, C):
    rng = np.random.default_rng(B * HW + C)
    A, dO = _channels(rng, B * HW, C, lo=0.5, hi=2.0).reshape(B, HW, C), _channels(rng, B * HW, C, lo=0.5, hi=2.0, offset=0.3).reshape(B, HW, C)
    g = rng.uniform(0, 1, (B, C)).astype(np.float32)
    dA_, dg_, dOut = ops.t(A), ops.t(g), ops.t(dO)
    mean, gA, gg = _new(ops, B, C), _new(ops, B, HW, C), _new(ops, B, C)
    ops.check(ops.L.mkws_op_pool_hw(ops.p(dA_), ops.p(mean), B, HW, C, ops.s()))
    assert _rel(_np(mean), A.astype(np.float64).mean(1)) < 1e-6
    ops.check(ops.L.mkws_op_se_bwd(ops.p(dA_), ops.p(dg_), ops.p(dOut), ops.p(gA), ops.p(gg), B, HW, C, ops.s()))
    assert _rel(_np(gA), dO.astype(np.float64) * g.astype(np.float64)[:, None]) < 1e-6
    assert _rel(_np(gg), (dO.astype(np.float64) * A.astype(np.float64)).sum(1)) < 1e-5


@pytest.mark.parametrize("HW,C,se", [(4, 1152, 48), (12, 40, 10)])        # nine full 128-channel slabs; C below one slab and no multiple of 64
@pytest.mark.parametrize("B", [64, 65, 129])                     # se_wgrad_kernel: one chunk of 64 clips (direct stores), two and three chunks (partial sums + four folds)
def test_squeeze_excite_across_the_batch_chunks(ops, B, HW, C, se):
    """mkws_op_se_fwd / mkws_op_se_bwd_fused against float64 autograd of pool -> dense(swish) -> dense(sigmoid) -> multiply, and mkws_op_se_wgrad on
    its own against the four sums it stands for."""
    chunks = _ceil(B, 64)
    assert chunks == {64: 1, 65: 2, 129: 3}[B] and (C < 128 or C % 128 == 0) and (C == 1152 or C % 64 != 0)
    rng = np.random.default_rng(B * 1000 + C)
    A = _channels(rng, B * HW, C, lo=0.5, hi=1.5, offset=0.3).reshape(B, HW, C)
    Wr, br = (rng.standard_normal((C, se)) / np.sqrt(C)).astype(np.float32), rng.standard_normal(se).astype(np.float32)
    We, be = (rng.standard_normal((se, C)) / np.sqrt(se)).astype(np.float32), rng.standard_normal(C).astype(np.float32)
    dO = rng.standard_normal((B, HW, C)).astype(np.float32)
    t64 = lambda a_: torch.tensor(a_, dtype=torch.float64, requires_grad=True)
    a, wr, b_r, we, b_e = t64(A), t64(Wr), t64(br), t64(We), t64(be)
    mean = a.mean(1)
    mean.retain_grad()
    yr = mean @ wr + b_r
    r = yr * torch.sigmoid(yr)
    g = torch.sigmoid(r @ we + b_e)
    out = a * g[:, None]
    (out * torch.tensor(dO, dtype=torch.float64)).sum().backward()
    dA_, dWr, dbr, dWe, dbe, ddO = ops.t(A), ops.t(Wr), ops.t(br), ops.t(We), ops.t(be), ops.t(dO)
    Mn, Yr, R, G, Out = _new(ops, B, C), _new(ops, B, se), _new(ops, B, se), _new(ops, B, C), _new(ops, B, HW, C)
    work = _new(ops, B, _ceil(C, 128) * se)
    ops.check(ops.L.mkws_op_se_fwd(ops.p(dA_), ops.p(dWr), ops.p(dbr), ops.p(dWe), ops.p(dbe), ops.p(Mn), ops.p(Yr), ops.p(R), ops.p(G), ops.p(Out),
                                   ops.p(work), B, HW, C, se, ops.s()))
    for got, ref, name in ((Mn, mean, "mean"), (Yr, yr, "Yr"), (R, r, "R"), (G, g, "G"), (Out, out, "out")):
        assert _rel(_np(got), ref.detach().numpy()) < 2e-6, name
    runs = []
    for _ in range(2):
        gA, gmean, gYg, gYr = _new(ops, B, HW, C), _new(ops, B, C), _new(ops, B, C), _new(ops, B, se)
        gWr, gbr, gWe, gbe = _new(ops, C, se), _new(ops, se), _new(ops, se, C), _new(ops, C)
        ops.check(ops.L.mkws_op_se_bwd_fused(ops.p(dA_), ops.p(G), ops.p(ddO), ops.p(Mn), ops.p(Yr), ops.p(R), ops.p(dWr), ops.p(dWe), ops.p(gA), ops.p(gmean),
                                             ops.p(gYg), ops.p(gYr), ops.p(gWr), ops.p(gbr), ops.p(gWe), ops.p(gbe), ops.p(work), B, HW, C, se, ops.s()))
        runs.append((gA, gmean, gYg, gYr, gWr, gbr, gWe, gbe))
    gA, gmean, gYg, gYr, gWr, gbr, gWe, gbe = runs[0]
    # dA is the multiply's direct path only; the squeeze's path (dmean / HW on every pixel) is added by the BatchNorm backward that follows
    assert _rel(_np(gA), dO.astype(np.float64) * g.detach().numpy()[:, None]) < 2e-6
    assert _rel(_np(gmean), mean.grad.numpy()) < 2e-5
    assert _rel(_np(gA).astype(np.float64) + _np(gmean)[:, None] / HW, a.grad.numpy()) < 2e-5
    for got, ref, name in ((gWr, wr.grad, "dWr"), (gbr, b_r.grad, "dbr"), (gWe, we.grad, "dWe"), (gbe, b_e.grad, "dbe")):
        assert _rel(_np(got), ref.numpy()) < 2e-5, name
    assert all(torch.equal(p, q) for p, q in zip(runs[0], runs[1]))       # fixed-order sums: a second call is bit-identical
    # the weight gradient on its own: dWr = mean^T dYr, dbr = colsum(dYr), dWe = R^T dYg, dbe = colsum(dYg), batch rows in chunks of 64
    mn, rr = _channels(rng, B, C, lo=0.5, hi=1.5, offset=0.3), _channels(rng, B, se, lo=0.5, hi=1.5, offset=0.3)
    dyg, dyr = _channels(rng, B, C, lo=0.5, hi=1.5, offset=0.3), _channels(rng, B, se, lo=0.5, hi=1.5, offset=0.3)
    d_mn, d_rr, d_dyg, d_dyr = ops.t(mn), ops.t(rr), ops.t(dyg), ops.t(dyr)
    f64 = lambda a_: a_.astype(np.float64)
    refs = (f64(mn).T @ f64(dyr), f64(dyr).sum(0), f64(rr).T @ f64(dyg), f64(dyg).sum(0))
    alone = []
    for _ in range(2):
        oWr, obr, oWe, obe = _new(ops, C, se), _new(ops, se), _new(ops, se, C), _new(ops, C)
        ops.check(ops.L.mkws_op_se_wgrad(ops.p(d_mn), ops.p(d_rr), ops.p(d_dyg), ops.p(d_dyr), ops.p(oWr), ops.p(obr), ops.p(oWe), ops.p(obe), B, C, se, ops.s()))
        alone.append((oWr, obr, oWe, obe))
    for got, ref, name in zip(alone[0], refs, ("dWr", "dbr", "dWe", "dbe")):
        assert _rel(_np(got), ref) < 2e-5, ("se_wgrad", name)
    assert all(torch.equal(p, q) for p, q in zip(alone[0], alone[1]))
