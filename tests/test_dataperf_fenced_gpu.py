"""The nine C entry points of the dataperf solvers (mkws_logreg_fit / _score, mkws_svc_prepare / _kernel / _fit / _score, mkws_kmeans_fit /
_nearest, mkws_roc_count) called straight through the library with every pointer argument in a fenced buffer of its own
(tests/util_fenced.py): inputs filled, outputs and workspaces holding the canary NaN, the workspace exactly as large as the library asks.

`protocol` (tests/util_fenced.py) is the one function that makes the assertions, for every entry point:
  1  the call returns 0 and every pad of every buffer is intact;
  2  every input is bit-identical to its snapshot;
  3  every element of the written set (include/mkws.h, built by util_fenced) no longer holds the canary and has the bits the Python
     wrapper returns for the same inputs -- or, where a wrapper does not expose an output, the bits of the same C call on ordinary
     zero-filled buffers (`reference` says which); where the contract says NaN the element is a NaN that is not the canary;
  4  every element outside the written set still holds what it held before the call;
  5  every written float is finite unless the contract says NaN;
  6  the same call again, into the now dirty outputs and workspace, gives the same bits, and so does a repeat after a call of another
     shape has used the same workspace allocation;
  7  (calls with a workspace) with one element too few the call is refused with MKWS_ERR_INVALID_ARG and every buffer is as it was.
Nothing is asserted about a workspace's contents after a call, only about its pads: "unspecified" is the contract.
An in-out argument (d_info and d_gap of mkws_svc_fit, which mkws_svc_prepare starts) is an output whose middle starts as what the
earlier call left in a canary-filled buffer; it is put back to that before every repeat, as an input would be.

In every bank, each row that no fitted problem's list names is the canary NaN, for the fenced call and for the reference alike."""
import functools

import numpy as np
import pytest

import util_fenced as uf
from util_fenced import Out, canaried, holds_canary, protocol

pytestmark = pytest.mark.gpu

SVC_TOL, SVC_MAX_ITER = 1e-5, 100000               # the wrapper's defaults, those of tests/test_svc_gpu.py
LOGREG_MAX_ITER, LOGREG_GTOL = 300, 1e-5           # the wrapper's defaults
KMEANS_MAX_ITER, KMEANS_TOL = 300, 1e-4


# ------------------------------------------------------------------------------------------------ plumbing

def _L():
    from multilingual_kws_amd import _lib
    return _lib.lib(), _lib.current_stream_ptr()


def plain(shape, dtype):
    """An ordinary zero-filled device buffer (never of no elements)."""
    import torch
    n = max(int(np.prod(shape, dtype=np.int64)), 1)
    return torch.zeros(n, dtype=getattr(torch, np.dtype(dtype).name), device="cuda")


def up(a):
    """A host array on the device, bit for bit (never of no elements)."""
    import torch
    a = np.ascontiguousarray(a).reshape(-1)
    if a.size == 0:
        a = np.zeros(1, a.dtype)
    return torch.from_numpy(a.view(np.int32).copy()).cuda().view(getattr(torch, a.dtype.name))


def down(t, shape, dtype):
    n = int(np.prod(shape, dtype=np.int64))
    return t.cpu().numpy()[:n].view(np.dtype(dtype)).reshape(shape).copy()


def addresses(tensors):
    return {k: (v.data_ptr() if v is not None else None) for k, v in tensors.items()}


def exact(a, b, what):
    assert np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes(), f"the wrapper and the C call on zero-filled buffers differ in {what}"


class Shape:
    """The scalar arguments of a solver case."""

    def __init__(self, c):
        self.n_bank, self.dim = (int(v) for v in c["x"].shape)
        self.P, self.K = len(c["offsets"]) - 1, int(c["n_classes"])
        self.npairs = self.K * (self.K - 1) // 2
        self.n_list, self.total = len(c["rows"]), len(c["score_rows"])
        self.max_rows = int(np.diff(c["offsets"]).max())
        self.max_eval = int(np.diff(c["score_offsets"]).max())
        self.standardize = int(bool(c["standardize"]))


# ---- the C calls, on a dict of addresses (fenced or ordinary) ----

def c_svc_prepare(s, p):
    L, st = _L()
    return L.mkws_svc_prepare(p["x"], s.n_bank, s.dim, p["rows"], p["labels"], p["offsets"], s.P, s.K, s.max_rows, s.standardize, 0.0, p["centre"],
                              p["inv_scale"], p["gamma"], p["info"], p["gap"], st)


def c_svc_kernel(s, p, max_a, max_b, out_stride, out="out"):
    L, st = _L()
    return L.mkws_svc_kernel(p["x"], s.n_bank, s.dim, p["rows_a"], p["offsets_a"], max_a, p["rows_b"], p["offsets_b"], max_b, s.P, p["centre"],
                             p["inv_scale"], p["gamma"], p["info"], p[out], out_stride, st)


def c_svc_fit(s, p, gram_stride):
    L, st = _L()
    return L.mkws_svc_fit(p["labels"], p["offsets"], s.P, s.K, s.max_rows, p["C"], SVC_TOL, SVC_MAX_ITER, p["gram"], gram_stride, p["coef"], p["rho"],
                          p["info"], p["gap"], st)


def c_svc_score(s, p):
    L, st = _L()
    return L.mkws_svc_score(p["x"], s.n_bank, s.dim, p["rows"], p["labels"], p["offsets"], s.max_rows, p["coef"], p["rho"], p["gamma"], p["centre"],
                            p["inv_scale"], p["info"], s.P, s.K, p["score_rows"], p["score_true"], p["score_offsets"], s.total, s.max_eval, p["pred"],
                            p["correct"], p["decision"], st)


def c_logreg_fit(s, p, work_floats):
    L, st = _L()
    return L.mkws_logreg_fit(p["x"], s.n_bank, s.dim, p["rows"], p["labels"], p["offsets"], s.P, s.K, p["C"], s.standardize, LOGREG_MAX_ITER,
                             LOGREG_GTOL, p["coef"], p["intercept"], p["info"], p["stats"], p["work"], work_floats, st)


def c_logreg_score(s, p):
    L, st = _L()
    return L.mkws_logreg_score(p["x"], s.n_bank, s.dim, p["score_rows"], p["score_true"], p["score_offsets"], s.P, s.K, p["coef"], p["intercept"],
                               s.total, p["pred"], p["probs"], p["logits"], p["correct"], st)


# ---- a small call of another shape, into somebody else's workspace ----

@functools.lru_cache(None)
def _other():
    """One problem of 4 rows, 2 classes and 5 columns, on the device."""
    rng = np.random.default_rng(11)
    return dict(x=up(rng.standard_normal((4, 5)).astype(np.float32)), rows=up(np.arange(4, dtype=np.int32)), labels=up(np.asarray([0, 1, 0, 1], np.int32)),
                offsets=up(np.asarray([0, 4], np.int32)), C=up(np.ones(1)), out=plain(256, np.float64))


def other_logreg_fit(work):
    """mkws_logreg_fit of the other shape with `work` (an address) as its workspace of 3 * 1 * 2 * 5 floats."""
    L, st = _L()
    o = addresses(_other())
    q = o["out"]                                                       # coef [2, 5], intercept [2], info [4], stats [2]
    rc = L.mkws_logreg_fit(o["x"], 4, 5, o["rows"], o["labels"], o["offsets"], 1, 2, o["C"], 0, 50, 1e-5, q, q + 128, q + 192, q + 256, work, 30, st)
    assert rc == 0 and L.mkws_logreg_work_floats(5, 1, 2) == 30


def other_svc_gram(work):
    """mkws_svc_prepare and mkws_svc_kernel of the other shape, the Gram matrix of 4 x 4 floats written at `work` (an address)."""
    L, st = _L()
    o = addresses(_other())
    q = o["out"]                                                       # centre [5], inv_scale [5], gamma, info [4], gap
    assert L.mkws_svc_prepare(o["x"], 4, 5, o["rows"], o["labels"], o["offsets"], 1, 2, 4, 0, 0.0, q, q + 32, q + 64, q + 96, q + 128, st) == 0
    assert L.mkws_svc_kernel(o["x"], 4, 5, o["rows"], o["offsets"], 4, o["rows"], o["offsets"], 4, 1, q, q + 32, q + 64, q + 96, work, 16, st) == 0


# ------------------------------------------------------------------------------------------------ the references, one per case

@functools.lru_cache(None)
def svc_reference(name):
    """Everything the five svc tests compare with, computed once: the wrappers' results on the poisoned bank, and the C calls on ordinary
    zero-filled buffers for what the wrappers do not expose (what mkws_svc_prepare alone leaves in info and gap, the Gram matrices, a
    cross-kernel of all problems at once).  Where both exist they are asserted equal here, byte for byte."""
    import torch
    from multilingual_kws_amd import svc
    c = uf.solver_case("svc", name)
    s = Shape(c)
    status = c["status"]
    named = uf.named_rows(s.n_bank, (c["rows"], c["offsets"], status), (c["score_rows"], c["score_offsets"], status))
    x = uf.poisoned_bank(c["x"], named)
    r = dict(x=x, shape=s)
    # the wrappers
    fit = svc.fit_on_device(x, c["rows"], c["labels"], c["offsets"], s.K, C=c["C"], standardize=c["standardize"], tol=SVC_TOL, max_iter=SVC_MAX_ITER)
    assert fit.info[:, 0].tolist() == status.tolist(), (name, fit.info)
    d_x = torch.from_numpy(x.copy()).cuda()
    pred, correct, dec = svc.score_on_device(d_x, c["score_rows"], c["score_true"], c["score_offsets"], c["rows"], c["labels"], c["offsets"], s.K,
                                             fit.d_coef, fit.d_rho, fit.d_gamma, fit.d_centre, fit.d_inv_scale, info=fit.d_info, want_decision=True)
    r.update(fit=fit, pred=pred.cpu().numpy(), correct=correct.cpu().numpy(), decision=dec.cpu().numpy())
    # the C calls on zero-filled buffers
    t = dict(x=d_x, rows=up(c["rows"]), labels=up(c["labels"]), offsets=up(c["offsets"]), C=up(c["C"]), score_rows=up(c["score_rows"]),
             score_offsets=up(c["score_offsets"]), centre=plain((s.P, s.dim), np.float32), inv_scale=plain((s.P, s.dim), np.float32),
             gamma=plain(s.P, np.float32), info=plain((s.P, 4), np.int32), gap=plain(s.P, np.float32), coef=plain((s.n_list, s.K - 1), np.float32),
             rho=plain((s.P, s.npairs), np.float32), gram=plain((s.P, s.max_rows ** 2), np.float32),
             cross=plain((s.P, s.max_rows * s.max_eval), np.float32))
    p = addresses(t)
    p.update(rows_a=p["rows"], offsets_a=p["offsets"])
    assert c_svc_prepare(s, p) == 0
    torch.cuda.synchronize()
    r["prep_info"], r["prep_gap"] = down(t["info"], (s.P, 4), np.int32), down(t["gap"], (s.P,), np.float32)
    assert c_svc_kernel(s, dict(p, rows_b=p["rows"], offsets_b=p["offsets"]), s.max_rows, s.max_rows, s.max_rows ** 2, out="gram") == 0
    assert c_svc_kernel(s, dict(p, rows_b=p["score_rows"], offsets_b=p["score_offsets"]), s.max_rows, s.max_eval, s.max_rows * s.max_eval, out="cross") == 0
    assert c_svc_fit(s, p, s.max_rows ** 2) == 0
    torch.cuda.synchronize()
    r["gram"], r["cross"] = down(t["gram"], (s.P, s.max_rows ** 2), np.float32), down(t["cross"], (s.P, s.max_rows * s.max_eval), np.float32)
    for part, shape, dtype in (("coef", (s.n_list, s.K - 1), np.float32), ("rho", (s.P, s.npairs), np.float32), ("gamma", (s.P,), np.float32),
                               ("centre", (s.P, s.dim), np.float32), ("inv_scale", (s.P, s.dim), np.float32), ("info", (s.P, 4), np.int32),
                               ("gap", (s.P,), np.float32)):
        exact(getattr(fit, part), down(t[part], shape, dtype), f"{name}: {part}")
    if s.P <= 3:                                                       # the one-problem kernel wrapper, problem by problem
        for q in np.nonzero(status == 0)[0]:
            a = c["rows"][c["offsets"][q]:c["offsets"][q + 1]]
            e = c["score_rows"][c["score_offsets"][q]:c["score_offsets"][q + 1]]
            for rows_b, got in ((a, r["gram"][q]), (e, r["cross"][q])):
                k = svc.kernel_on_device(d_x, a, rows_b, fit.d_centre[q], fit.d_inv_scale[q], float(fit.gamma[q])).cpu().numpy()
                exact(k, got[:k.size].reshape(k.shape), f"{name}: the kernel values of problem {q}")
    return r


@functools.lru_cache(None)
def logreg_reference(name):
    import torch
    from multilingual_kws_amd import logreg
    c = uf.solver_case("logreg", name)
    s = Shape(c)
    status = c["status"]
    named = uf.named_rows(s.n_bank, (c["rows"], c["offsets"], status), (c["score_rows"], c["score_offsets"], status))
    x = uf.poisoned_bank(c["x"], named)
    fit = logreg.fit_on_device(x, c["rows"], c["labels"], c["offsets"], s.K, C=c["C"], standardize=c["standardize"], max_iter=LOGREG_MAX_ITER,
                               gtol=LOGREG_GTOL)
    assert fit.info[:, 0].tolist() == status.tolist(), (name, fit.info)
    r = dict(x=x, shape=s, fit=fit)
    if not status.any():
        out = logreg.score_on_device(torch.from_numpy(x.copy()).cuda(), c["score_rows"], c["score_true"], c["score_offsets"], fit.d_coef, fit.d_intercept,
                                     want_probs=True, want_logits=True)
        r["pred"], r["correct"], r["probs"], r["logits"] = (v.cpu().numpy() for v in out)
    return r


# ------------------------------------------------------------------------------------------------ logistic regression

@pytest.mark.parametrize("name", uf.LOGREG_CASES)
def test_logreg_fit(name):
    pytest.importorskip("torch")
    c, r = uf.solver_case("logreg", name), logreg_reference(name)
    s, fit = r["shape"], r["fit"]
    L, _ = _L()
    n_work = int(L.mkws_logreg_work_floats(s.dim, s.P, s.K))
    assert n_work == 3 * s.P * s.K * s.dim
    w = uf.logreg_fit_written(c["offsets"], c["status"], s.K, s.dim)
    inputs = dict(x=r["x"], rows=c["rows"], labels=c["labels"], offsets=c["offsets"], C=c["C"])
    outputs = {k: Out(getattr(fit, k), w[k]) for k in ("coef", "intercept", "info", "stats")}
    got = protocol(lambda p: c_logreg_fit(s, p, n_work), inputs, outputs, work_floats=n_work, refused=lambda p: c_logreg_fit(s, p, n_work - 1),
                   other_shape=lambda p: other_logreg_fit(p["work"]))
    for q in np.nonzero(c["status"] == 2)[0]:
        assert got["info"][q].tolist() == [2, 0, 0, int(c["offsets"][q + 1] - c["offsets"][q])]


@pytest.mark.parametrize("name", [n for n in uf.LOGREG_CASES if "+" not in n])
def test_logreg_score(name):
    """The coefficients arrive as the fit leaves them in a canary-filled buffer.  (The refused variants are not scored: this scorer takes no
    d_info, and what a refused problem's coefficients hold is not specified.)"""
    pytest.importorskip("torch")
    c, r = uf.solver_case("logreg", name), logreg_reference(name)
    s, fit = r["shape"], r["fit"]
    w = uf.logreg_fit_written(c["offsets"], c["status"], s.K, s.dim)
    outside = uf.outside_entries(c["score_rows"], c["score_offsets"], s.n_bank)
    assert outside[:2].all() and outside[-2:].all() and outside.sum() == 5 and (r["pred"][outside] == -1).all() and (r["pred"][~outside] >= 0).all()
    sw = uf.score_written(s.total, s.P, s.K, second="logits")
    inputs = dict(x=r["x"], score_rows=c["score_rows"], score_true=c["score_true"], score_offsets=c["score_offsets"],
                  coef=canaried(fit.coef, w["coef"]), intercept=canaried(fit.intercept, w["intercept"]))
    outputs = dict(pred=Out(r["pred"], sw["pred"]), probs=Out(r["probs"], sw["values"], nan=outside[:, None]),
                   logits=Out(r["logits"], sw["logits"], nan=outside[:, None]), correct=Out(r["correct"], sw["correct"]))
    got = protocol(lambda p: c_logreg_score(s, p), inputs, outputs)
    off = c["score_offsets"]
    assert got["correct"].tolist() == [int((got["pred"][off[q]:off[q + 1]] == c["score_true"][off[q]:off[q + 1]]).sum()) for q in range(s.P)]


# ------------------------------------------------------------------------------------------------ support-vector classifiers

@pytest.mark.parametrize("name", uf.SVC_CASES)
def test_svc_prepare(name):
    pytest.importorskip("torch")
    c, r = uf.solver_case("svc", name), svc_reference(name)
    s, fit = r["shape"], r["fit"]
    w = uf.svc_prepare_written(c["offsets"], c["status"], s.dim)
    inputs = dict(x=r["x"], rows=c["rows"], labels=c["labels"], offsets=c["offsets"])
    outputs = dict(centre=Out(fit.centre, w["centre"]), inv_scale=Out(fit.inv_scale, w["inv_scale"]), gamma=Out(fit.gamma, w["gamma"]),
                   info=Out(r["prep_info"], w["info"]), gap=Out(r["prep_gap"], w["gap"]))
    got = protocol(lambda p: c_svc_prepare(s, p), inputs, outputs)
    ok = c["status"] == 0
    assert not got["gap"][ok].any() and not got["info"][ok][:, 2:].any() and (got["info"][~ok] == [2, 0, 0, 0]).all()


def _prepared(c, r):
    """centre, inv_scale, gamma, info and gap as mkws_svc_prepare leaves them in canary-filled buffers."""
    s, fit = r["shape"], r["fit"]
    w = uf.svc_prepare_written(c["offsets"], c["status"], s.dim)
    return dict(centre=canaried(fit.centre, w["centre"]), inv_scale=canaried(fit.inv_scale, w["inv_scale"]), gamma=canaried(fit.gamma, w["gamma"]),
                info=canaried(r["prep_info"], w["info"]), gap=canaried(r["prep_gap"], w["gap"]))


@pytest.mark.parametrize("cross", [False, True], ids=["gram", "cross"])
@pytest.mark.parametrize("name", uf.SVC_CASES)
def test_svc_kernel(name, cross):
    """gram: both lists the training lists, as in a fit, the output a workspace of exactly mkws_svc_work_bytes.  cross: list A the training
    lists, list B the evaluation lists (na != nb, and the B offsets start behind two entries that no list names)."""
    pytest.importorskip("torch")
    c, r = uf.solver_case("svc", name), svc_reference(name)
    s = r["shape"]
    L, _ = _L()
    rows_b, offsets_b, max_b, want = (c["score_rows"], c["score_offsets"], s.max_eval, r["cross"]) if cross else (c["rows"], c["offsets"], s.max_rows, r["gram"])
    stride = s.max_rows * max_b
    if not cross:
        assert int(L.mkws_svc_work_bytes(s.P, s.max_rows)) == 4 * s.P * stride
    else:
        assert (np.diff(offsets_b) != np.diff(c["offsets"])).all()
    w = uf.svc_kernel_written(c["offsets"], offsets_b, c["status"], stride)
    pre = _prepared(c, r)
    del pre["gap"]
    inputs = dict(x=r["x"], rows_a=c["rows"], offsets_a=c["offsets"], rows_b=rows_b, offsets_b=offsets_b, **pre)
    nan = uf.svc_kernel_nan(c["rows"], c["offsets"], rows_b, offsets_b, c["status"], s.n_bank, stride)
    assert int(nan.sum()) == (int(np.diff(c["offsets"])[0]) if cross else 0)   # problem 0's evaluation list ends in a row outside the bank: one NaN column
    outputs = dict(out=Out(want.reshape(-1), w["out"], nan=nan))
    protocol(lambda p: c_svc_kernel(s, p, s.max_rows, max_b, stride), inputs, outputs, refused=lambda p: c_svc_kernel(s, p, s.max_rows, max_b, stride - 1),
             other_shape=lambda p: other_svc_gram(p["out"]))


@pytest.mark.parametrize("name", uf.SVC_CASES)
def test_svc_fit(name):
    """The Gram matrices arrive as mkws_svc_kernel leaves them in a canary-filled workspace of exactly mkws_svc_work_bytes: n_p * n_p floats
    at the head of every slot of max_rows^2, the canary NaN behind them and in the whole slot of a refused problem.  For the repeat "after
    another shape" a 4 x 4 Gram matrix of another problem is written into the workspace by a real call, the canary elsewhere is replaced by
    a stale but plausible kernel value (0.75), and the case's own matrices are put back over their n_p * n_p floats."""
    pytest.importorskip("torch")
    c, r = uf.solver_case("svc", name), svc_reference(name)
    s, fit = r["shape"], r["fit"]
    L, _ = _L()
    stride = s.max_rows ** 2
    assert int(L.mkws_svc_work_bytes(s.P, s.max_rows)) == 4 * s.P * stride
    gw = uf.svc_kernel_written(c["offsets"], c["offsets"], c["status"], stride)["out"]
    gram = canaried(r["gram"].reshape(-1), gw)
    stale = np.where(gw, r["gram"].reshape(-1), np.float32(0.75)).astype(np.float32)
    pre = _prepared(c, r)
    w = uf.svc_fit_written(c["offsets"], c["status"], s.n_list, s.K)
    inputs = dict(labels=c["labels"], offsets=c["offsets"], C=c["C"], gram=gram)
    outputs = dict(coef=Out(fit.coef, w["coef"]), rho=Out(fit.rho, w["rho"]), info=Out(fit.info, w["info"], start=pre["info"]),
                   gap=Out(fit.gap, w["gap"], start=pre["gap"]))

    def other_shape(p):
        other_svc_gram(p["gram"])
        return dict(gram=stale)
    got = protocol(lambda p: c_svc_fit(s, p, stride), inputs, outputs, refused=lambda p: c_svc_fit(s, p, stride - 1), other_shape=other_shape)
    if name == "n150_k2_dim37":
        assert got["info"][0, :3].tolist() == [0, 1, 0] and got["info"][0, 3] >= 1 and got["gap"][0] < SVC_TOL, (got["info"], got["gap"])
    if name == "absent_class":                                         # the zero coefficients and rho of pairs with the absent class are written
        assert (got["coef"] == 0).any(axis=0).all() and (got["rho"][0] == 0).sum() == 3


@pytest.mark.parametrize("name", uf.SVC_CASES)
def test_svc_score(name):
    """The model arrives as prepare and fit leave it in canary-filled buffers: the coefficient rows of list entries that no offset names, and
    everything of a refused problem but its info, hold the canary NaN."""
    pytest.importorskip("torch")
    c, r = uf.solver_case("svc", name), svc_reference(name)
    s, fit = r["shape"], r["fit"]
    pre = _prepared(c, r)
    w = uf.svc_fit_written(c["offsets"], c["status"], s.n_list, s.K)
    outside = uf.outside_entries(c["score_rows"], c["score_offsets"], s.n_bank, c["status"])
    assert outside[:2].all() and outside[-2:].all() and (r["pred"][outside] == -1).all() and (r["pred"][~outside] >= 0).all()
    sw = uf.score_written(s.total, s.P, s.npairs)
    inputs = dict(x=r["x"], rows=c["rows"], labels=c["labels"], offsets=c["offsets"], coef=canaried(fit.coef, w["coef"]), rho=canaried(fit.rho, w["rho"]),
                  gamma=pre["gamma"], centre=pre["centre"], inv_scale=pre["inv_scale"], info=fit.info, score_rows=c["score_rows"],
                  score_true=c["score_true"], score_offsets=c["score_offsets"])
    outputs = dict(pred=Out(r["pred"], sw["pred"]), decision=Out(r["decision"], sw["values"], nan=outside[:, None]), correct=Out(r["correct"], sw["correct"]))
    got = protocol(lambda p: c_svc_score(s, p), inputs, outputs)
    off = c["score_offsets"]
    assert got["correct"].tolist() == [int((got["pred"][off[q]:off[q + 1]] == c["score_true"][off[q]:off[q + 1]]).sum()) for q in range(s.P)]


# ------------------------------------------------------------------------------------------------ k-means

@functools.lru_cache(None)
def kmeans_reference(name):
    """mkws_kmeans_fit and mkws_kmeans_nearest on ordinary zero-filled buffers (the wrapper refuses a group shorter than n_clusters before
    anything is uploaded), and the wrappers on the bank of the fitted groups alone, asserted equal group by group."""
    import torch
    from multilingual_kws_amd import kmeans
    c = uf.kmeans_case(name)
    off, k, status = c["offsets"], c["k"], c["status"]
    n_rows, dim = c["x"].shape
    G, T = len(status), kmeans.n_local_trials(k)
    in_fitted = np.zeros(n_rows, bool)
    for g in np.nonzero(status != 2)[0]:
        in_fitted[off[g]:off[g + 1]] = True
    x = uf.poisoned_bank(c["x"], in_fitted)
    draws = np.stack([kmeans.kmeans_draws(seed, k) for seed in c["seeds"]])
    t = dict(x=up(x), offsets=up(off), draws=up(draws), centers=plain((G, k, dim), np.float32), centers_f64=plain((G, k, dim), np.float64),
             labels=plain(n_rows, np.int32), init=plain((G, k), np.int32), info=plain((G, 4), np.int32))
    p = addresses(t)
    r = dict(x=x, draws=draws, T=T)
    assert c_kmeans_fit(c, T, p) == 0
    torch.cuda.synchronize()
    for part, shape, dtype in (("centers", (G, k, dim), np.float32), ("centers_f64", (G, k, dim), np.float64), ("labels", (n_rows,), np.int32),
                               ("init", (G, k), np.int32), ("info", (G, 4), np.int32)):
        r[part] = down(t[part], shape, dtype)
    assert r["info"][:, 0].tolist() == status.tolist(), r["info"]
    keep = [g for g in range(G) if status[g] != 2]
    sub = np.concatenate([x[off[g]:off[g + 1]] for g in keep])
    sub_off = np.concatenate([[0], np.cumsum([off[g + 1] - off[g] for g in keep])])
    fit = kmeans.kmeans_fit_on_device(sub, sub_off, k, [c["seeds"][g] for g in keep], max_iter=KMEANS_MAX_ITER, tol=KMEANS_TOL, want_f64=True)
    for i, g in enumerate(keep):
        exact(fit.info[i], r["info"][g], f"{name}: info of group {g}")
        if status[g] == 0:
            for part in ("centers", "centers_f64", "init"):
                exact(getattr(fit, part)[i], r[part][g], f"{name}: {part} of group {g}")
            exact(fit.labels[sub_off[i]:sub_off[i + 1]], r["labels"][off[g]:off[g + 1]], f"{name}: labels of group {g}")
    # nearest: every row of a fitted group against its own group's centres, the others under a group index outside [0, G)
    w, _ = uf.kmeans_fit_written(off, status, k, dim, n_rows)
    read = (c["group"] >= 0) & (c["group"] < G)
    r["near_x"] = uf.poisoned_bank(c["x"], read)
    r["near_centers"] = canaried(r["centers"], w["centers"])
    dist, which, invalid = kmeans.nearest_on_device(up(r["near_x"]).view(n_rows, dim), c["group"].copy(), up(np.where(w["centers"], r["centers"], np.float32(0))).view(G, k, dim))
    r["dist"], r["which"], r["invalid"] = dist.cpu().numpy(), which.cpu().numpy(), invalid.cpu().numpy()
    return r


def c_kmeans_fit(c, T, p):
    L, st = _L()
    return L.mkws_kmeans_fit(p["x"], c["x"].shape[1], p["offsets"], len(c["status"]), c["k"], p["draws"], T, KMEANS_MAX_ITER, KMEANS_TOL, p["centers"],
                             p["centers_f64"], p["labels"], p["init"], p["info"], st)


@pytest.mark.parametrize("name", list(uf.KMEANS_CASES))
def test_kmeans_fit(name):
    pytest.importorskip("torch")
    c, r = uf.kmeans_case(name), kmeans_reference(name)
    n_rows, dim = c["x"].shape
    w, loose = uf.kmeans_fit_written(c["offsets"], c["status"], c["k"], dim, n_rows)
    inputs = dict(x=r["x"], offsets=c["offsets"], draws=r["draws"])
    outputs = {k: Out(r[k], w[k], unspecified=loose[k]) for k in ("centers", "centers_f64", "labels", "init", "info")}
    got = protocol(lambda p: c_kmeans_fit(c, r["T"], p), inputs, outputs)
    assert (got["info"][c["status"] == 2] == [2, 0, 0, 0]).all()
    for g in np.nonzero(c["status"] == 1)[0]:
        assert got["info"][g, 0] == 1 and got["info"][g, 1] >= 1 and not got["info"][g, 2:].any()
    assert holds_canary(got["labels"])[:c["offsets"][0]].all() and holds_canary(got["labels"])[c["offsets"][-1]:].all()


@pytest.mark.parametrize("name", list(uf.KMEANS_CASES))
def test_kmeans_nearest(name):
    """The centres arrive as the fit leaves them in a canary-filled buffer (a refused group's hold the canary NaN); rows of groups that were
    not fitted, and rows outside every group, carry a group index outside [0, G) and are the canary NaN in the bank."""
    pytest.importorskip("torch")
    c, r = uf.kmeans_case(name), kmeans_reference(name)
    n_rows, dim = c["x"].shape
    G, k = len(c["status"]), c["k"]
    L, st = _L()
    w = uf.kmeans_nearest_written(n_rows)
    bad = (c["group"] < 0) | (c["group"] >= G)
    assert bad.sum() >= 3 and {-1, G, 2 ** 30} <= set(c["group"][bad].tolist()) and r["invalid"].tolist() == [int(bad.sum())]
    inputs = dict(x=r["near_x"], group=c["group"], centers=r["near_centers"])
    outputs = dict(dist=Out(r["dist"], w["dist"], nan=bad), which=Out(r["which"], w["which"]), invalid=Out(r["invalid"].astype(np.int32), w["invalid"]))
    got = protocol(lambda p: L.mkws_kmeans_nearest(p["x"], dim, n_rows, p["group"], p["centers"], G, k, p["dist"], p["which"], p["invalid"], st), inputs, outputs)
    assert (got["which"][bad] == -1).all() and (got["which"][~bad] >= 0).all()


# ------------------------------------------------------------------------------------------------ ROC counts

@pytest.mark.parametrize("n_thr,mode", [(1, 0), (257, 0), (4096, 0), (257, 1)])
def test_roc_count(n_thr, mode):
    """Four heads: one without negatives, one without positives, one with both, one with neither (its counts are written zeros).  Every row
    of a head's plane that neither of its lists names is the canary NaN."""
    torch = pytest.importorskip("torch")
    from multilingual_kws_amd.roc import pack_rows, roc_counts_on_device
    probs, pos, neg = uf.roc_case()
    H, N, C = probs.shape
    thr = uf.roc_thresholds(n_thr)
    assert thr.size == n_thr and (np.diff(thr) > 0).all()
    probs = probs.copy()
    for h in range(H):
        named = np.zeros(N, bool)
        named[pos[h] + neg[h]] = True
        assert not named.all()
        probs[h].view(np.int32)[~named] = uf.CANARY
    counts, totals = roc_counts_on_device(torch.from_numpy(probs.copy()).cuda(), pos, neg, thr, target_id=2, multiclass=bool(mode), negative_class=1)
    assert totals.tolist() == [[len(a), len(b)] for a, b in zip(pos, neg)] and totals[3].tolist() == [0, 0] and counts[:3].any()
    (pos_rows, pos_off), (neg_rows, neg_off) = pack_rows(pos, H, N, "positives"), pack_rows(neg, H, N, "negatives")
    w = uf.roc_written(H, n_thr)
    L, st = _L()
    inputs = dict(probs=probs, pos_rows=pos_rows, pos_offsets=pos_off, neg_rows=neg_rows, neg_offsets=neg_off, thresholds=thr)
    outputs = dict(counts=Out(counts, w["counts"]), invalid=Out(np.zeros(H, np.int32), w["invalid"]))
    got = protocol(lambda p: L.mkws_roc_count(p["probs"], H, N, C, p["pos_rows"], p["pos_offsets"], p["neg_rows"], p["neg_offsets"], p["thresholds"], n_thr,
                                              mode, 2, 1, p["counts"], p["invalid"], st), inputs, outputs)
    assert not got["counts"][3].any() and not got["counts"][0, :, 1].any() and not got["counts"][1, :, 0].any()
