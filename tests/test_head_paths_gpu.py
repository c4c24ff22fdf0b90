"""-m gpu: every launch path of the few-shot head (mkws_head.hip) against oracle/head_oracle.py in float64.

Both forward kernels at every K-split edge, tile count, hidden parity and class count; the multi-head launches; loss, statistics
and every gradient block at the ragged row slices and widths the product creates; the input gradient's grid-stride loop; both Adam
kernels; the argument checks.  Tolerances are multiples of the oracle's own float32 round-off (tests/util_head.py), the case tables
are the ones tests/test_head_checks_cpu.py vets without a device.

MKWS_HEAD_ACCURACY_OUT=<file> writes measured error / round-off unit of every comparison (profiles/head_paths_accuracy.txt)."""
import ctypes
import os
import time

import numpy as np
import pytest

from tests import util_head as uh

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def heads(dev):
    """One Head per dimension triple, reused across regimes and batch sizes (set_params also clears the optimizer state)."""
    from multilingual_kws_amd.head import Head
    cache, t0 = {}, time.perf_counter()

    def get(dims):
        if dims not in cache:
            cache[dims] = Head(*dims, max_batch=uh.MAX_BATCH, seed=0, device=dev)
        return cache[dims]

    yield get
    torch.cuda.synchronize()
    for hd in cache.values():
        hd.close()
    out = os.environ.get("MKWS_HEAD_ACCURACY_OUT")
    if out:
        uh.write_records(out, "%.1f s from the first head to the last test of the file, %d comparisons" % (time.perf_counter() - t0, len(uh.RECORDS)))


def dev_case(case, dev):
    return torch.from_numpy(case.x).to(dev), torch.from_numpy(case.y).to(dev)


# ---- a, d: forward, single head -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("spec", uh.forward_cases(), ids=uh.case_id)
def test_forward(dev, heads, spec):
    case = uh.forward_case(*spec)
    hd = heads(case.dims)
    hd.set_params(case.p)
    x, _ = dev_case(case, dev)
    full = hd.forward(x)
    assert full.shape == (case.B, case.dims[2])
    uh.check_probs(full.cpu().numpy(), case)
    for b in uh.FORWARD_PREFIXES:                       # a row depends on nothing but itself: the 16-row tile and 4-rows-per-workgroup edges
        assert torch.equal(hd.forward(x[:b]), full[:b]), (case.id, b)
    assert torch.equal(hd.forward(x), full), case.id


# ---- b: forward, many heads -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dims", uh.MANY_HEADS_CASES, ids=uh.case_id)
def test_forward_many(dev, dims):
    from multilingual_kws_amd.head import Head
    case, params = uh.many_heads_case(dims)
    hs = [Head(*dims, max_batch=64, params=p, device=dev) for p in params]
    x = torch.from_numpy(case.x).to(dev)
    try:
        for B in uh.MANY_HEADS_BATCHES:
            xb = x[:B]
            single = [h.forward(xb) for h in hs]
            for n in uh.MANY_HEADS_COUNTS:
                many = Head.forward_many(hs[:n], xb)
                assert many.shape == (n, B, dims[2])
                assert torch.equal(many, torch.stack(single[:n])), (dims, B, n)
        assert B == case.B
        uh.check_probs(single[0].cpu().numpy(), case)               # the first head against the oracle
        assert Head.forward_many(hs[:3], x[:0]).shape == (3, 0, dims[2])
    finally:
        for h in hs:
            h.close()


def test_forward_many_refuses_unequal_heads(dev):
    from multilingual_kws_amd._lib import MkwsError
    from multilingual_kws_amd.head import Head
    x = torch.zeros((4, 192), dtype=torch.float32, device=dev)
    a = Head(192, 16, 3, max_batch=8, seed=0, device=dev)
    for other in ((192, 15, 3), (192, 16, 2), (208, 16, 3)):
        b = Head(*other, max_batch=8, seed=1, device=dev)
        with pytest.raises(MkwsError):
            Head.forward_many([a, b], x)
        with pytest.raises(MkwsError):
            Head.forward_many([a, a, b], x)
        b.close()
    assert Head.forward_many([a, a], x).shape == (2, 4, 3)
    a.close()


# ---- c, d: loss, statistics, gradient ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("spec", uh.grad_cases(), ids=uh.case_id)
def test_loss_statistics_gradient(dev, heads, spec):
    case = uh.Case(*spec[0], *spec[1:])
    hd = heads(case.dims)
    hd.set_params(case.p)
    x, y = dev_case(case, dev)
    stats = hd.loss_grad(x, y).cpu().numpy().copy()
    g = hd.grad_view(with_stats=True).cpu().numpy().copy()
    assert g.shape == (hd.nparams + 2,) and np.all(np.isfinite(g))
    assert np.array_equal(g[-2:], stats)                            # the all-reduce payload carries the returned statistics
    uh.check_loss_sum(stats[0], case)
    uh.check_ncorrect(stats[1], case)
    uh.check_gradient(g[:-2], case)
    stats2 = hd.loss_grad(x, y).cpu().numpy()
    assert np.array_equal(hd.grad_view(with_stats=True).cpu().numpy(), g) and np.array_equal(stats2, stats)      # fixed-order reductions
    uh.check_probs(hd.forward(x).cpu().numpy(), case)               # the inference kernel at this batch size and label-free


# ---- e: input gradient --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("spec", uh.INPUT_GRAD_CASES, ids=uh.case_id)
def test_input_grad(dev, heads, spec):
    dims, B, regime = spec
    case = uh.Case(*dims, B, regime)
    hd = heads(dims)
    hd.set_params(case.p)
    x, y = dev_case(case, dev)
    hd.loss_grad(x, y)
    dx = hd.input_grad(B)
    assert dx.shape == (B, dims[0])
    uh.assert_close(dx.cpu().numpy(), case, "dX")
    assert torch.equal(hd.input_grad(B), dx)


# ---- f: Adam ------------------------------------------------------------------------------------------------------------------------

def run_adam(dev, ac, variant):
    """The device trajectory of an AdamCase through adam_step (host step index) or adam_step_dev (device step word)."""
    from multilingual_kws_amd.head import Head
    o = ac.opts
    hd = Head(*ac.dims, max_batch=uh.ADAM_BATCH, params=ac.p0, device=dev)
    step = torch.zeros(1, dtype=torch.int32, device=dev)
    hd.step_t = ac.first_t - 1
    for i, (x, y) in enumerate(ac.batches):
        hd.loss_grad(torch.from_numpy(x).to(dev), torch.from_numpy(y).to(dev))
        if variant == "host":
            hd.adam_step(lr=uh.ADAM_LR, beta1=o["beta1"], beta2=o["beta2"], eps=o["eps"], grad_scale=o["grad_scale"])
        else:
            step.fill_(ac.first_t + i)
            hd.adam_step_dev(uh.ADAM_LR, step, beta1=o["beta1"], beta2=o["beta2"], eps=o["eps"], grad_scale=o["grad_scale"])
    if variant == "host":
        assert hd.step_t == ac.first_t - 1 + len(ac.batches)
    p = hd.get_params()
    hd.close()
    return p


@pytest.mark.parametrize("setting", sorted(uh.ADAM_SETTINGS))
@pytest.mark.parametrize("first_t,steps", [(1, uh.ADAM_STEPS), (1000, 1), (100000, 1)])
def test_adam_both_kernels(dev, setting, first_t, steps):
    ac = uh.AdamCase(setting, steps=steps, first_t=first_t)
    host, devp = run_adam(dev, ac, "host"), run_adam(dev, ac, "dev")
    ac.assert_close(host)
    ac.assert_close(devp)
    # the two kernels differ only in where lr_t is evaluated (host libm / device, both in double, rounded to float32 once):
    # measured bit-equal on the MI355X in all six cases, so that is what is pinned
    assert np.array_equal(host, devp), (ac.id, np.abs(host.astype(np.float64) - devp).max())
    still = ac.untouched()
    assert np.array_equal(host[still], ac.p0[still]) and np.array_equal(devp[still], ac.p0[still])        # zero gradient: bit-unchanged
    assert np.mean(np.delete(host, still) != np.delete(ac.p0, still)) > 0.99


# ---- g: error contract (host-side argument checks only: nothing here reaches a launch with a bad argument) ---------------------------

def test_error_contract(dev):
    from multilingual_kws_amd import _lib
    from multilingual_kws_amd.head import Head
    E = _lib.MkwsError
    for bad in ((0, 18, 3), (-16, 18, 3), (1024, 18, 1), (1024, 18, 9), (1024, 0, 3), (1024, 33, 3)):
        with pytest.raises(E):
            Head(*bad, max_batch=8, seed=0, device=dev)
    with pytest.raises(E):
        Head(1024, 18, 3, max_batch=0, seed=0, device=dev)
    hd = Head(64, 5, 2, max_batch=8, seed=0, device=dev)
    p0 = hd.get_params()
    for n in (hd.nparams - 1, hd.nparams + 1, 0):
        with pytest.raises(E):
            hd.set_params(np.zeros(n, dtype=np.float32))
    assert np.array_equal(hd.get_params(), p0)
    x = torch.zeros((9, 64), dtype=torch.float32, device=dev)
    y = torch.zeros(9, dtype=torch.int32, device=dev)
    L, stream = _lib.lib(), _lib.current_stream_ptr()
    for t in (0, -1):
        with pytest.raises(E):
            _lib.check(L.mkws_head_adam_step(hd.h, 1e-3, 0.9, 0.999, 1e-7, t, 1.0, stream))
    with pytest.raises(E):
        hd.loss_grad(x[:0], y[:0])                   # B = 0
    with pytest.raises(E):
        hd.loss_grad(x, y)                           # B = 9 > max_batch = 8
    with pytest.raises(E):
        hd.input_grad(9)
    with pytest.raises(E):
        hd.input_grad(0)
    assert np.array_equal(hd.get_params(), p0)       # none of the refused calls touched the parameters
    # empty work is no error and launches nothing
    assert hd.forward(x[:0]).shape == (0, 2)
    assert Head.forward_many([hd, hd], x[:0]).shape == (2, 0, 2)
    out = torch.full((4,), 7.0, dtype=torch.float32, device=dev)
    table = (ctypes.c_void_p * 1)(hd.h.value)
    assert _lib.check(L.mkws_heads_forward(table, 0, ctypes.c_void_p(x.data_ptr()), 4, ctypes.c_void_p(out.data_ptr()), stream)) == 0
    with pytest.raises(E):
        _lib.check(L.mkws_heads_forward(table, -1, ctypes.c_void_p(x.data_ptr()), 4, ctypes.c_void_p(out.data_ptr()), stream))
    torch.cuda.synchronize()
    assert out.tolist() == [7.0] * 4
    hd.close()
