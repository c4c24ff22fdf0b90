"""mkws_svc_fit_cv, mkws_svc_platt, mkws_svc_couple and mkws_soft_vote under the protocol of tests/util_fenced.py (its docstring and that of
tests/test_dataperf_fenced_gpu.py number the assertions): every argument in a fenced buffer of exactly its size, outputs and workspaces
canary-filled, inputs arriving as the call before them leaves them in canary-filled buffers (the Gram workspace of mkws_svc_kernel, the
info of mkws_svc_prepare, the cv_decision of mkws_svc_fit_cv, ...).  Asserted: the return code, pads intact, inputs untouched, the written
set exactly what include/mkws.h says, no canary inside it, equal bytes with the wrappers' results and on a second call.

The written sets, from include/mkws.h:
  fit_cv   d_cv_info of every problem (zeroed by the call); d_cv_decision: all K - 1 values of every entry of a problem whose d_info and
           d_cv_info statuses are 0, nothing else;
  platt    d_probA[p], d_probB[p], d_present[p] of such a problem, nothing else;
  couple   all of d_probs, d_pred, d_correct; NaN probabilities where an entry is outside every list, its row outside the bank or its
           problem refused;
  vote     all of d_pred, d_correct, d_mean."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import util_fenced as uf  # noqa: E402
from util_fenced import Out, canaried, protocol  # noqa: E402

from multilingual_kws_amd import _lib, svc  # noqa: E402

pytestmark = pytest.mark.gpu

TOL, MAX_ITER, EPS, F = 1e-5, 100000, 1e-8, 5
NAMES = ["ragged_50_20_64", "ragged_50_20_64+label", "ragged_50_20_64+fold", "absent_class", "n150_k2_dim37", "65_problems_of_8_dim16"]


def _L():
    return _lib.lib(), _lib.current_stream_ptr()


@functools.lru_cache(None)
def reference(name):
    """The wrappers on ordinary buffers: the fit with its sigmoids, the Gram matrices problem by problem, the scores on the case's score lists."""
    import torch
    base, _, bad = name.partition("+")
    c = uf.solver_case("svc", base if bad == "fold" else name)
    off = c["offsets"]
    folds = svc.cv_folds(c["labels"], off, F, 3)
    status, cv_status = np.array(c["status"]), np.array(c["status"])
    if bad == "fold":
        folds[off[1] + 2] = -1
        cv_status[1] = 2
    d_x = torch.from_numpy(c["x"].copy()).cuda()
    fit = svc.fit_proba_on_device(d_x, c["rows"], c["labels"], off, c["n_classes"], folds=folds, n_folds=F, C=c["C"], standardize=c["standardize"],
                                  tol=TOL, max_iter=MAX_ITER, platt_eps=EPS)
    assert fit.info[:, 0].tolist() == status.tolist() and fit.cv_info[:, 0].tolist() == cv_status.tolist()
    P, K = len(off) - 1, int(c["n_classes"])
    max_rows = int(np.diff(off).max())
    gram = np.zeros((P, max_rows * max_rows), np.float32)
    for p in np.nonzero(status == 0)[0]:
        rows = c["rows"][off[p]:off[p + 1]]
        g = svc.kernel_on_device(d_x, rows, rows, fit.d_centre[p], fit.d_inv_scale[p], float(fit.gamma[p]))
        gram[p, :g.numel()] = g.cpu().numpy().reshape(-1)
    pred, correct, decision = svc.score_on_device(d_x, c["score_rows"], c["score_true"], c["score_offsets"], c["rows"], c["labels"], off, K, fit.d_coef,
                                                  fit.d_rho, fit.d_gamma, fit.d_centre, fit.d_inv_scale, info=fit.d_cv_info, want_decision=True)
    cp, cc, cprobs = svc.couple_on_device(decision, c["score_true"], c["score_offsets"], fit.d_probA, fit.d_probB, fit.d_present)
    other = torch.from_numpy(np.random.default_rng(1).dirichlet(np.ones(K), len(c["score_rows"])).astype(np.float32)).cuda()
    vp, vc, vm = svc.soft_vote_on_device(cprobs, other, c["score_true"], c["score_offsets"], want_mean=True)
    host = lambda t: t.cpu().numpy()
    return dict(c=c, folds=folds.astype(np.int32), status=status, cv_status=cv_status, fit=fit, gram=gram, max_rows=max_rows, P=P, K=K,
                decision=host(decision), couple=(host(cp), host(cc), host(cprobs)), other=host(other), vote=(host(vp), host(vc), host(vm)))


def entries_of(off, ok, n_list, width):
    out = np.zeros((n_list, width), bool)
    for p in np.nonzero(ok)[0]:
        out[off[p]:off[p + 1]] = True
    return out


@pytest.mark.parametrize("name", NAMES)
def test_svc_fit_cv(name):
    r = reference(name)
    c, fit, P, K, max_rows = r["c"], r["fit"], r["P"], r["K"], r["max_rows"]
    L, st = _L()
    off, stride = c["offsets"], max_rows * max_rows
    gw = uf.svc_kernel_written(off, off, r["status"], stride)["out"]
    info = canaried(fit.info, np.ones((P, 4), bool))
    inputs = dict(labels=c["labels"], offsets=off, folds=r["folds"], C=c["C"], gram=canaried(r["gram"].reshape(-1), gw), info=info)
    outputs = dict(cv_decision=Out(fit.cv_decision, entries_of(off, r["cv_status"] == 0, len(c["rows"]), K - 1)),
                   cv_info=Out(fit.cv_info, np.ones((P, 4), bool)))

    def call(p, gram_stride=stride):
        return L.mkws_svc_fit_cv(p["labels"], p["offsets"], p["folds"], F, P, K, max_rows, p["C"], TOL, MAX_ITER, p["gram"], gram_stride, p["info"],
                                 p["cv_decision"], p["cv_info"], st)
    got = protocol(call, inputs, outputs, refused=lambda p: call(p, stride - 1))
    assert got["cv_info"][:, 0].tolist() == r["cv_status"].tolist() and not got["cv_info"][r["cv_status"] != 0, 1:].any()


@pytest.mark.parametrize("name", NAMES)
def test_svc_platt(name):
    r = reference(name)
    c, fit, P, K = r["c"], r["fit"], r["P"], r["K"]
    L, st = _L()
    off, ok = c["offsets"], r["cv_status"] == 0
    npairs = K * (K - 1) // 2
    inputs = dict(labels=c["labels"], offsets=off, cv_decision=canaried(fit.cv_decision, entries_of(off, ok, len(c["rows"]), K - 1)),
                  info=canaried(fit.info, np.ones((P, 4), bool)), cv_info=fit.cv_info)
    wide = np.broadcast_to(ok[:, None], (P, npairs))
    outputs = dict(probA=Out(fit.probA, wide), probB=Out(fit.probB, wide), present=Out(fit.present, ok))
    protocol(lambda p: L.mkws_svc_platt(p["labels"], p["offsets"], P, K, r["max_rows"], p["cv_decision"], p["info"], p["cv_info"], EPS, p["probA"],
                                        p["probB"], p["present"], st), inputs, outputs)


@pytest.mark.parametrize("name", NAMES)
def test_svc_couple_and_soft_vote(name):
    r = reference(name)
    c, fit, P, K = r["c"], r["fit"], r["P"], r["K"]
    L, st = _L()
    ok = r["cv_status"] == 0
    npairs, total = K * (K - 1) // 2, len(c["score_rows"])
    outside = uf.outside_entries(c["score_rows"], c["score_offsets"], c["x"].shape[0], r["cv_status"])
    pred, correct, probs = r["couple"]
    assert (pred[outside] == -1).all() and (pred[~outside] >= 0).all() and np.isnan(probs[outside]).all() and np.isfinite(probs[~outside]).all()
    wide = np.broadcast_to(ok[:, None], (P, npairs))
    inputs = dict(decision=r["decision"], true=c["score_true"], offsets=c["score_offsets"], probA=canaried(fit.probA, wide),
                  probB=canaried(fit.probB, wide), present=canaried(fit.present, ok))
    outputs = dict(probs=Out(probs, True, nan=outside[:, None]), pred=Out(pred, True), correct=Out(correct, True))
    protocol(lambda p: L.mkws_svc_couple(p["decision"], p["true"], p["offsets"], P, K, total, p["probA"], p["probB"], p["present"], p["probs"],
                                         p["pred"], p["correct"], st), inputs, outputs)
    vp, vc, vm = r["vote"]
    assert (vp[outside] == -1).all() and (vp[~outside] >= 0).all()
    inputs = dict(a=probs, b=r["other"], true=c["score_true"], offsets=c["score_offsets"])
    outputs = dict(pred=Out(vp, True), correct=Out(vc, True), mean=Out(vm, True, nan=outside[:, None]))
    got = protocol(lambda p: L.mkws_soft_vote(p["a"], p["b"], p["true"], p["offsets"], P, K, total, p["pred"], p["correct"], p["mean"], st), inputs, outputs)
    so = c["score_offsets"]
    assert got["correct"].tolist() == [int((got["pred"][so[q]:so[q + 1]] == c["score_true"][so[q]:so[q + 1]]).sum()) for q in range(P)]
