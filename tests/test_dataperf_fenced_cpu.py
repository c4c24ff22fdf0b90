"""The tools of tests/test_dataperf_fenced_gpu.py, checked without a device: the fenced buffers and the protocol (tests/util_fenced.py) see a
store into a pad, an unwritten element, a store outside the written set, a changed input and a result that depends on what the workspace
or the outputs held, on CPU tensors and with small host functions in the place of the C calls; and for every case of the GPU file the
written-set masks have the counts that the sentences of include/mkws.h give."""
import ctypes

import numpy as np
import pytest

import util_fenced as uf
from util_fenced import CANARY, PAD, FencedBuffer, Out, canaried, canary_array, holds_canary, protocol, same_bits


# ------------------------------------------------------------------------------------------------ the buffers

@pytest.mark.parametrize("dtype", uf.DTYPES)
def test_a_fresh_buffer_is_canary_everywhere_and_its_views_are_typed(dtype):
    pytest.importorskip("torch")
    f = FencedBuffer(5, dtype, device="cpu")
    k = np.dtype(dtype).itemsize // 4
    assert f.whole.numel() == 2 * PAD + 5 * k and f.mid.numel() == 5 and str(f.mid.dtype).endswith(dtype)
    assert f.ptr() == f.whole.data_ptr() + 4 * PAD and f.ptr() % 8 == 0
    assert f.pads_intact() and f.canary_mask().all() and f.host().dtype == np.dtype(dtype)
    assert (f.whole.numpy() == CANARY).all()
    if dtype == "float32":
        assert np.isnan(f.host()).all()                                # a read of it poisons
    if dtype == "float64":
        assert (f.host() > 1e307).all()                                # two canary words are 2.25e307: finite, and no value of these solvers
    empty = FencedBuffer(0, dtype, device="cpu")
    assert empty.pads_intact() and empty.canary_mask().shape == (0,) and empty.ptr() == empty.whole.data_ptr() + 4 * PAD


def test_a_store_into_either_pad_is_seen():
    pytest.importorskip("torch")
    for dtype in uf.DTYPES:
        k = np.dtype(dtype).itemsize // 4
        for word in (0, PAD - 1, PAD + 7 * k, 2 * PAD + 7 * k - 1):
            f = FencedBuffer(7, dtype, device="cpu")
            f.whole[word] = 0
            assert not f.pads_intact() and f.canary_mask().all(), (dtype, word)
        f = FencedBuffer(7, dtype, device="cpu")
        f.whole[PAD] = 0
        f.whole[PAD + 7 * k - 1] = 0
        assert f.pads_intact() and f.canary_mask().tolist() == [False] + [True] * 5 + [False]


def test_an_unwritten_element_and_a_changed_input_are_seen():
    torch = pytest.importorskip("torch")
    f = FencedBuffer(6, "float64", device="cpu")
    f.mid[1] = 0.0                                                     # a written zero is not the canary
    f.words[2 * 4] = 0                                                 # half of element 4 written: not the canary either
    assert f.canary_mask().tolist() == [True, False, True, True, False, True]
    values = np.asarray([1.5, -0.0, np.nan, 3.0], np.float32)
    g = FencedBuffer(4, "float32", fill=values, device="cpu")
    assert g.host().tobytes() == values.tobytes() and not g.canary_mask().any() and g.pads_intact()
    snap = g.snapshot()
    assert g.unchanged_since(snap)
    g.mid[1] = 0.0                                                     # -0.0 -> +0.0: equal as numbers, not as bits
    assert not g.unchanged_since(snap)
    g.fill(values)
    assert g.unchanged_since(snap)
    g.whole[3] = 1                                                     # a pad belongs to the snapshot
    assert not g.unchanged_since(snap)
    with pytest.raises(ValueError):
        g.fill(values.astype(np.float64))
    with pytest.raises(ValueError):
        g.fill(values[:3])
    h = FencedBuffer(3, "int64", fill=np.asarray([1, -1, 2 ** 40]), device="cpu")
    assert h.host().tolist() == [1, -1, 2 ** 40] and torch.equal(h.mid, torch.tensor([1, -1, 2 ** 40]))
    h.reset()
    assert h.canary_mask().all()


def test_host_helpers():
    c = canary_array((2, 3), np.float64)
    assert holds_canary(c).all() and np.isnan(c.view(np.float32)).all() and canary_array(4, np.int32).tolist() == [CANARY] * 4
    v = np.arange(6, dtype=np.float32).reshape(2, 3)
    m = v % 2 == 0
    k = canaried(v, m)
    assert (holds_canary(k) == ~m).all() and (k[m] == v[m]).all()
    assert same_bits(np.float32([0.0, np.nan]), np.float32([-0.0, np.nan])).tolist() == [False, True]


# ------------------------------------------------------------------------------------------------ the protocol, on host functions

def _floats(address, n):
    return np.ctypeslib.as_array((ctypes.c_float * n).from_address(address))


N, WRITTEN = 9, np.arange(9) % 3 != 2            # the toy call writes out[i] = 2 x[i] + 1 where i % 3 != 2, through a workspace of N floats


def _toy(flaw=None):
    calls = []

    def call(p, n_work=N):
        if n_work < N:
            if flaw == "refusal writes":
                _floats(p["work"], 1)[0] = 0.0
            return uf.INVALID_ARG
        x, out, work = _floats(p["x"], N), _floats(p["out"], N + 1), _floats(p["work"], N)
        stale = float(work[0])
        work[:] = 2 * x
        for i in np.nonzero(WRITTEN)[0]:
            if flaw == "skips one" and i == 7:
                continue
            out[i] = work[i] + 1
        if flaw == "reads the workspace":
            out[0] += 0 * stale                                        # right when the workspace held a finite value, NaN when it held the canary
        if flaw == "one too many":
            out[8] = 0.0
        if flaw == "into the pad":
            out[N] = 0.0
        if flaw == "changes an input":
            x[4] = x[4] + 1
        if flaw == "accumulates" and calls:
            out[0] = out[0] + 1
        if flaw == "remembers the workspace" and len(calls) == 2:
            out[1] = 0.0
        calls.append(1)
        return 0
    return call


def _run_toy(flaw, **kw):
    x = np.linspace(-1, 1, N).astype(np.float32)
    call = _toy(flaw)
    return protocol(call, dict(x=x), dict(out=Out(2 * x + 1, WRITTEN)), work_floats=N, refused=lambda p: call(p, N - 1),
                    other_shape=lambda p: _floats(p["work"], 3).fill(7.0), device="cpu", **kw)


def test_protocol_passes_a_call_that_keeps_its_contract():
    pytest.importorskip("torch")
    got = _run_toy(None)
    assert holds_canary(got["out"]).tolist() == (~WRITTEN).tolist()


@pytest.mark.parametrize("flaw,message", [("skips one", "inside its written set: 1 elements, the first at \\(7,\\)"),
                                          ("one too many", "written outside its written set: 1 elements, the first at \\(8,\\)"),
                                          ("into the pad", "a pad of out was written"),
                                          ("changes an input", "the input x changed"),
                                          ("reads the workspace", "holds the canary \\(never written, or computed from a canary NaN, whose payload travels\\)"),
                                          ("accumulates", "second call: out differs from the reference"),
                                          ("remembers the workspace", "call after another shape: out differs from the reference"),
                                          ("refusal writes", "the refused call changed work")])
def test_protocol_sees_every_kind_of_breach(flaw, message):
    pytest.importorskip("torch")
    with pytest.raises(AssertionError, match=message):
        _run_toy(flaw)


def test_protocol_in_out_arguments_nan_and_unspecified_elements():
    pytest.importorskip("torch")
    start = np.asarray([5, 0, 0, CANARY], np.int32)

    def call(p):
        info = np.ctypeslib.as_array((ctypes.c_int32 * 4).from_address(p["info"]))
        info[2] += 3                                                   # doubles if the protocol does not put the start back
        val = _floats(p["val"], 3)
        val[0], val[1] = np.nan, np.random.default_rng().random()      # val[1] is unspecified: it may differ from call to call
        return 0
    info_written = np.asarray([False, False, True, False])
    outs = lambda nan: dict(info=Out(np.asarray([0, 0, 3, 0], np.int32), info_written, start=start),
                            val=Out(np.zeros(3, np.float32), [True, False, False], nan=nan, unspecified=[False, True, False]))
    got = protocol(call, {}, outs([True, False, False]), device="cpu")
    assert got["info"].tolist() == [5, 0, 3, CANARY] and np.isnan(got["val"][0]) and holds_canary(got["val"])[2]
    with pytest.raises(AssertionError, match="val is not finite"):
        protocol(call, {}, outs(None), device="cpu")                    # a NaN where the contract does not say NaN


# ------------------------------------------------------------------------------------------------ the written sets of the GPU file's cases

def _sizes(c, key="offsets"):
    return np.diff(c[key]).astype(np.int64)


@pytest.mark.parametrize("family,name", [("svc", n) for n in uf.SVC_CASES] + [("logreg", n) for n in uf.LOGREG_CASES])
def test_solver_masks_have_the_counts_of_their_formulas(family, name):
    c = uf.solver_case(family, name)
    n, ne, status = _sizes(c), _sizes(c, "score_offsets"), c["status"]
    ok = status == 0
    P, K, dim, n_bank = len(n), c["n_classes"], c["x"].shape[1], c["x"].shape[0]
    n_list, total = len(c["rows"]), len(c["score_rows"])
    assert status.tolist() == ([0, 2, 0] if "+" in name else [0] * P) and int(ok.sum()) == P - ("+" in name)
    assert total == c["score_offsets"][-1] + 2 and c["score_offsets"][0] == 2 and (ne == n + (4 if "65_" in name else 60 if "k6_" in name else 16)).all()
    if family == "logreg":
        w = uf.logreg_fit_written(c["offsets"], status, K, dim)
        assert {k: v.shape for k, v in w.items()} == dict(coef=(P, K, dim), intercept=(P, K), stats=(P, 2), info=(P, 4))
        assert [int(w[k].sum()) for k in ("coef", "intercept", "stats", "info")] == [ok.sum() * K * dim, ok.sum() * K, ok.sum() * 2, 4 * P]
        assert not w["coef"][~ok].any() and w["coef"][ok].all()
        outside = uf.outside_entries(c["score_rows"], c["score_offsets"], n_bank)
        assert outside.sum() == 5 and outside[[0, 1, c["score_offsets"][1] - 1, -2, -1]].all()
    else:
        w = uf.svc_prepare_written(c["offsets"], status, dim)
        assert [int(w[k].sum()) for k in ("centre", "inv_scale", "gamma", "info", "gap")] == [ok.sum() * dim, ok.sum() * dim, ok.sum(), 4 * P, ok.sum()]
        stride = int(n.max()) ** 2
        g = uf.svc_kernel_written(c["offsets"], c["offsets"], status, stride)["out"].reshape(P, stride)
        assert g.sum(axis=1).tolist() == np.where(ok, n * n, 0).tolist()                      # n_p^2 Gram words per fitted problem, 0 for a refused one
        for p in range(P):
            assert g[p, :n[p] * n[p] * ok[p]].all() and not g[p, n[p] * n[p] * ok[p]:].any()  # tight at the head of the slot, the tail untouched
        stride = int(n.max()) * int(ne.max())
        x = uf.svc_kernel_written(c["offsets"], c["score_offsets"], status, stride)["out"].reshape(P, stride)
        assert x.sum(axis=1).tolist() == np.where(ok, n * ne, 0).tolist()
        w = uf.svc_fit_written(c["offsets"], status, n_list, K)
        assert w["coef"].shape == (n_list, K - 1) and int(w["coef"].sum()) == int((n[ok] * (K - 1)).sum())
        assert int(w["rho"].sum()) == ok.sum() * K * (K - 1) // 2 and int(w["info"].sum()) == 2 * ok.sum() and int(w["gap"].sum()) == ok.sum()
        assert not w["info"][:, :2].any() and not w["coef"][:c["offsets"][0]].any() and not w["coef"][c["offsets"][-1]:].any()
        outside = uf.outside_entries(c["score_rows"], c["score_offsets"], n_bank, status)
        assert outside.sum() == 5 + ne[~ok].sum() and outside[c["score_offsets"][1] - 1] and c["score_rows"][c["score_offsets"][1] - 1] == n_bank
        nan = uf.svc_kernel_nan(c["rows"], c["offsets"], c["score_rows"], c["score_offsets"], status, n_bank, stride).reshape(P, stride)
        assert nan.sum() == n[0] and nan[0, ne[0] - 1:n[0] * ne[0]:ne[0]].all() and not (nan & ~x).any()    # one NaN column, in problem 0
        assert not uf.svc_kernel_nan(c["rows"], c["offsets"], c["rows"], c["offsets"], status, n_bank, int(n.max()) ** 2).any()
        sw = uf.score_written(total, P, K * (K - 1) // 2)
        assert [int(sw[k].sum()) for k in ("pred", "values", "correct")] == [total, total * K * (K - 1) // 2, P]
    # the bank: a row that no fitted problem's list names is the canary NaN, the others keep their bits
    named = uf.named_rows(n_bank, (c["rows"], c["offsets"], status), (c["score_rows"], c["score_offsets"], status))
    x = uf.poisoned_bank(c["x"], named)
    assert holds_canary(x)[~named].all() and x[named].tobytes() == c["x"][named].tobytes() and np.isfinite(x[named]).all()
    want = np.zeros(n_bank, bool)
    for p in np.nonzero(ok)[0]:
        for rows, off in ((c["rows"], c["offsets"]), (c["score_rows"], c["score_offsets"])):
            r = rows[off[p]:off[p + 1]]
            want[r[r < n_bank]] = True
    assert (named == want).all()
    if name.startswith("ragged"):
        assert not named[:3].any() and not named[-2:].any() and len(c["rows"]) == c["offsets"][-1] + 2 and c["offsets"][0] == 3
        assert int((~named).sum()) == 5 + 1 + (0 if ok.all() else 20 + 16)   # the lead and tail rows, the row the bad entry replaced, a refused problem's rows
    if "+row" in name:
        assert c["rows"][c["offsets"][2] - 1] == n_bank
    if "+label" in name:
        assert c["labels"][c["offsets"][1] + 5] == K


def test_the_new_svc_case_leaves_the_lds_cache_and_has_a_ragged_third_tile():
    c = uf.solver_case("svc", "n150_k2_dim37")
    assert c["x"].shape == (166, 37) and c["n_classes"] == 2 and c["offsets"].tolist() == [0, 150]
    assert np.bincount(c["labels"]).tolist() == [75, 75]              # its single pair has m = 150 rows: above the 128 that SMO keeps in LDS
    assert [min(64, 150 - t) for t in range(0, 150, 64)] == [64, 64, 22] and 37 % 4 and 37 % 16


@pytest.mark.parametrize("name", list(uf.KMEANS_CASES))
def test_kmeans_masks_have_the_counts_of_their_formulas(name):
    c = uf.kmeans_case(name)
    dim, k, parts = uf.KMEANS_CASES[name]
    off, status = c["offsets"], c["status"]
    n = np.diff(off)
    n_rows, G = c["x"].shape[0], len(status)
    assert n_rows == sum(m for _, m in parts) and status.tolist() == [{"good": 0, "short": 2, "same": 1}[kind] for kind, _ in parts if kind != "loose"]
    assert (n[status == 2] < k).all() and (n[status != 2] >= k).all() and off[0] > 0 and off[-1] < n_rows and 2 in status[1:-1]
    ok, loose = status == 0, status == 1
    w, u = uf.kmeans_fit_written(off, status, k, dim, n_rows)
    assert [int(w[p].sum()) for p in ("centers", "centers_f64", "labels", "init", "info")] == [ok.sum() * k * dim] * 2 + [n[ok].sum(), ok.sum() * k, 4 * G]
    assert [int(u[p].sum()) for p in ("centers", "centers_f64", "labels", "init", "info")] == [loose.sum() * k * dim] * 2 + [n[loose].sum(), loose.sum() * k, 0]
    assert not w["labels"][:off[0]].any() and not w["labels"][off[-1]:].any() and not (w["labels"] & u["labels"]).any()
    for g in range(G):
        assert w["labels"][off[g]:off[g + 1]].all() == bool(ok[g]) and w["centers"][g].all() == bool(ok[g])
        assert (c["group"][off[g]:off[g + 1]] == (g if ok[g] else -1)).all()
    outside = np.r_[0:off[0], off[-1]:n_rows]
    assert set(c["group"][outside].tolist()) <= {-1, G, 2 ** 30} and len(outside) >= 3
    nw = uf.kmeans_nearest_written(n_rows)
    assert [int(v.sum()) for v in nw.values()] == [n_rows, n_rows, 1]


def test_roc_masks_and_case():
    probs, pos, neg = uf.roc_case()
    assert probs.shape == (4, 63, 3) and [bool(p) for p in pos] == [True, False, True, False] and [bool(q) for q in neg] == [False, True, True, False]
    for n_thr in uf.ROC_THRESHOLDS:
        thr = uf.roc_thresholds(n_thr)
        w = uf.roc_written(4, n_thr)
        assert thr.size == n_thr and (np.diff(thr) > 0).all() and int(w["counts"].sum()) == 4 * n_thr * 2 and int(w["invalid"].sum()) == 4
    assert uf.ROC_THRESHOLDS == [1, 257, 4096]
