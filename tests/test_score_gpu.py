"""-m gpu: the point scorer (mkws_score_accumulate behind scoring.Scorer) against scoring.score_host on every case of
tests/score_cases.py.  Integers -- counters, confusion matrices, group tallies, predictions -- are compared with ==; row losses and
their sums within the bound score_cases derives (measured, four times the kernel-order twin's distance from exact arithmetic; see its
docstring).  Then the call's contracts: the same bits on every run, the same integers however the rows are cut into calls, a row's loss
independent of its batch, optional outputs that change nothing, every buffer between canaries, graph replay, empty calls, invalid labels."""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest

from multilingual_kws_amd import _lib, scoring
from tests import score_cases as sc

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

CASES = sc.all_cases()
_built, _measured = {}, {"row0": 0.0, "row1": 0.0, "sum": 0.0}


def built(case):
    """The case's arrays and its float64 specification, computed once and shared (nothing modifies them)."""
    if case["name"] not in _built:
        scores, labels, groups, named = sc.build(case)
        _built[case["name"]] = (scores, labels, groups, sc.host(case, scores, labels, groups))
    return _built[case["name"]]


def on_device(case, scores, labels, groups, cuts=(), optional=True, confusion=True):
    """One Scorer over the case, the rows cut into calls at `cuts` -> (raw accumulators, pred [K, N], row_loss [K, N])."""
    K, N, C = scores.shape
    scorer = scoring.Scorer(K, C, case["mode"], n_groups=case["n_groups"], confusion=confusion)
    d_scores, d_labels = torch.from_numpy(scores).cuda(), torch.from_numpy(labels).cuda()
    d_groups = torch.from_numpy(groups).cuda() if groups is not None else None
    preds, losses = [], []
    edges = [0] + list(cuts) + [N]
    for a, b in zip(edges, edges[1:]):
        pred = torch.full((K, b - a), -7, dtype=torch.int32, device="cuda") if optional else None
        loss = torch.full((K, b - a), 123.0, dtype=torch.float64, device="cuda") if optional else None
        scorer.add(d_scores[:, a:b], d_labels[..., a:b], d_groups[a:b] if d_groups is not None else None, row_loss=loss, pred=pred)
        preds.append(pred)
        losses.append(loss)
    raw = scorer.raw()
    if not optional:
        return raw, None, None
    return raw, torch.cat(preds, 1).cpu().numpy(), torch.cat(losses, 1).cpu().numpy()


def assert_integers(raw, want, pred=None):
    assert np.array_equal(raw.tally, want.tally), (raw.tally, want.tally)
    if raw.confusion is not None:
        assert np.array_equal(raw.confusion, want.confusion)
    assert np.array_equal(raw.group_tally, want.group_tally)
    if pred is not None:
        assert np.array_equal(pred, want.pred)


def assert_losses(case, scores, want, raw, row_loss=None):
    """Non-finite losses agree in kind; finite ones within the derived bounds.  -> the largest distances seen, in units."""
    row_bound, sum_bound = sc.loss_bounds(case, scores, want)
    seen = dict(row=0.0, sum=0.0)
    finite = np.isfinite(want.row_loss)
    if row_loss is not None:
        assert np.array_equal(np.isnan(row_loss), np.isnan(want.row_loss))
        assert np.array_equal(row_loss[~finite & ~np.isnan(want.row_loss)], want.row_loss[~finite & ~np.isnan(want.row_loss)])     # infinities
        err = np.abs(row_loss[finite] - want.row_loss[finite])
        if err.size:
            seen["row"] = float((err / (row_bound[finite] / sc.ROW_BOUND_UNITS[case["mode"]])).max())
            print(f"{case['name']}: largest row distance {seen['row']:.3f} units (allowed {sc.ROW_BOUND_UNITS[case['mode']]})")
        assert np.all(err <= row_bound[finite]), (case["name"], float((err / row_bound[finite]).max()))
    for k in range(scores.shape[0]):
        if np.isfinite(want.loss_sum[k]):
            err = abs(raw.loss_sum[k] - want.loss_sum[k])
            scale = sc.EPS * np.abs(want.row_loss[k][finite[k]]).sum()
            if scale > 0:
                seen["sum"] = max(seen["sum"], float(err / scale))
            assert err <= sum_bound[k], (case["name"], k, raw.loss_sum[k], want.loss_sum[k], sum_bound[k])
        else:
            assert np.isnan(raw.loss_sum[k]) if np.isnan(want.loss_sum[k]) else raw.loss_sum[k] == want.loss_sum[k], (case["name"], k)
    return seen


@pytest.mark.parametrize("case", CASES, ids=lambda c: c["name"])
def test_every_case_against_the_specification(case):
    scores, labels, groups, want = built(case)
    raw, pred, row_loss = on_device(case, scores, labels, groups)
    assert_integers(raw, want, pred)
    seen = assert_losses(case, scores, want, raw, row_loss)
    _measured[f"row{case['mode']}"] = max(_measured[f"row{case['mode']}"], seen["row"])
    _measured["sum"] = max(_measured["sum"], seen["sum"])
    print(f"so far, largest distances in units: {_measured}")


PICK = [c for c in CASES if c["rows"] in (257, 513, None) and c["classes"] in (3, 32, 33, 761)]


@pytest.mark.parametrize("case", PICK, ids=lambda c: c["name"])
def test_two_runs_give_the_same_bits_and_optional_outputs_change_nothing(case):
    scores, labels, groups, want = built(case)
    first, pred1, loss1 = on_device(case, scores, labels, groups)
    second, pred2, loss2 = on_device(case, scores, labels, groups)
    bare, _, _ = on_device(case, scores, labels, groups, optional=False, confusion=False)
    for other in (second, bare):
        assert first.loss_sum.view(np.int64).tolist() == other.loss_sum.view(np.int64).tolist()
        assert np.array_equal(first.tally, other.tally) and np.array_equal(first.group_tally, other.group_tally)
    assert np.array_equal(first.confusion, second.confusion) and bare.confusion is None
    assert np.array_equal(pred1, pred2) and np.array_equal(loss1.view(np.int64), loss2.view(np.int64))


@pytest.mark.parametrize("case", [c for c in PICK if c["rows"] == 513], ids=lambda c: c["name"])
def test_three_calls_at_unaligned_cuts_tally_what_one_call_tallies(case):
    scores, labels, groups, want = built(case)
    one, pred1, loss1 = on_device(case, scores, labels, groups)
    three, pred3, loss3 = on_device(case, scores, labels, groups, cuts=(37, 300))
    assert_integers(three, want, pred3)
    assert np.array_equal(one.tally, three.tally) and np.array_equal(one.confusion, three.confusion) and np.array_equal(one.group_tally, three.group_tally)
    assert np.array_equal(loss1.view(np.int64), loss3.view(np.int64))          # a row's loss does not depend on its batch
    assert_losses(case, scores, want, three, loss3)
    _, sum_bound = sc.loss_bounds(case, scores, want)
    for k in range(scores.shape[0]):
        if np.isfinite(want.loss_sum[k]):
            assert abs(one.loss_sum[k] - three.loss_sum[k]) <= 2 * sum_bound[k]


@pytest.mark.parametrize("case", [c for c in PICK if c["rows"] in (257, None)], ids=lambda c: c["name"])
def test_a_rows_loss_is_the_one_row_calls_loss(case):
    scores, labels, groups, want = built(case)
    _, pred, loss = on_device(case, scores, labels, groups)
    N = scores.shape[1]
    for r in sorted({0, 5, N // 2, N - 1}):
        lab = labels[..., r:r + 1]
        _, p1, l1 = on_device(case, np.ascontiguousarray(scores[:, r:r + 1]), np.ascontiguousarray(lab), groups[r:r + 1] if groups is not None else None)
        assert np.array_equal(l1.view(np.int64), loss[:, r:r + 1].view(np.int64)) and np.array_equal(p1, pred[:, r:r + 1]), r


CANARY = 0x7FC00BAD
PAD = 4096             # int32 words in front of and behind every buffer


def _fenced(n_bytes):
    """A CUDA buffer [PAD | n_bytes, rounded up to words | PAD] of canary words -> (whole, device pointer of the middle, words of the middle)."""
    words = (n_bytes + 3) // 4
    whole = torch.full((PAD + words + PAD,), CANARY, dtype=torch.int32, device="cuda")
    return whole, whole.data_ptr() + 4 * PAD, words


def _pads_intact(whole, words):
    return bool((whole[:PAD] == CANARY).all()) and bool((whole[PAD + words:] == CANARY).all())


@pytest.mark.parametrize("name", ["grid-C3-N513-mode0", "grid-C32-N257-mode1", "grid-C33-N257-mode0", "grid-C761-N65-mode1", "named-C3-mode0", "named-C761-mode1"])
def test_every_buffer_of_the_c_call_sits_between_canaries(name):
    case = next(c for c in CASES if c["name"] == name)
    scores, labels, groups, want = built(case)
    K, N, C = scores.shape
    G = case["n_groups"]
    L = _lib.lib()
    work_bytes = L.mkws_score_work_bytes(K, N)
    assert work_bytes == K * N * 8
    sizes = dict(scores=scores.nbytes, labels=labels.nbytes, groups=groups.nbytes if groups is not None else 0, loss=K * 8, tally=K * 32,
                 confusion=K * C * C * 8, group_tally=K * G * 16, row_loss=K * N * 8, pred=K * N * 4, work=work_bytes)
    buf = {k: _fenced(v) for k, v in sizes.items()}

    def fill(key, array):
        whole, _, words = buf[key]
        whole[PAD:PAD + words] = torch.from_numpy(np.ascontiguousarray(array).view(np.int32).reshape(-1)).cuda()

    fill("scores", scores)
    fill("labels", labels)
    if groups is not None:
        fill("groups", groups)
    for key in ("loss", "tally", "confusion", "group_tally"):
        buf[key][0][PAD:PAD + buf[key][2]] = 0
    ptr = lambda key: ctypes.c_void_p(buf[key][1])
    code = L.mkws_score_accumulate(ptr("scores"), K, N, C, case["mode"], ptr("labels"), int(labels.ndim == 2), ptr("groups") if groups is not None else None, G,
                                   ptr("loss"), ptr("tally"), ptr("confusion"), ptr("group_tally") if G else None, ptr("row_loss"), ptr("pred"), ptr("work"),
                                   _lib.current_stream_ptr())
    _lib.check(code)
    torch.cuda.synchronize()
    for key, (whole, _, words) in buf.items():
        assert _pads_intact(whole, words), f"a store outside {key}"
    mid = lambda key, dtype: buf[key][0][PAD:PAD + buf[key][2]].cpu().numpy().view(dtype)
    for key, array in (("scores", scores), ("labels", labels)):
        assert np.array_equal(mid(key, np.int32), np.ascontiguousarray(array).view(np.int32).reshape(-1)), f"{key} was written"
    raw = SimpleNamespace(loss_sum=mid("loss", np.float64), tally=mid("tally", np.int64).reshape(K, 4), confusion=mid("confusion", np.int64).reshape(K, C, C),
                                  group_tally=mid("group_tally", np.int64).reshape(K, G, 2))
    assert_integers(raw, want, mid("pred", np.int32).reshape(K, N))
    assert_losses(case, scores, want, raw, mid("row_loss", np.float64).reshape(K, N))
    work = mid("work", np.float64).reshape(K, N)                      # every word of the workspace is written: the loss, or 0 for an untallied row
    assert np.array_equal(np.isnan(work), np.isnan(want.row_loss) & (want.kind == 0)) and np.all(work[want.kind != 0] == 0.0)


def test_empty_calls_touch_nothing():
    L = _lib.lib()
    acc, p_acc, words = _fenced(1024)
    one, p_one, _ = _fenced(64)
    for K, N in ((0, 5), (3, 0), (0, 0)):
        _lib.check(L.mkws_score_accumulate(ctypes.c_void_p(p_one), K, N, 3, 0, ctypes.c_void_p(p_one), 0, None, 0, ctypes.c_void_p(p_acc), ctypes.c_void_p(p_acc + 64),
                                           ctypes.c_void_p(p_acc + 256), None, ctypes.c_void_p(p_acc + 512), ctypes.c_void_p(p_acc + 768), ctypes.c_void_p(p_one),
                                           _lib.current_stream_ptr()))
    torch.cuda.synchronize()
    assert bool((acc == CANARY).all()) and bool((one == CANARY).all())
    scorer = scoring.Scorer(2, 3, 0, n_groups=2)
    scorer.add(torch.zeros((2, 0, 3), device="cuda"), torch.zeros(0, dtype=torch.int32, device="cuda"), torch.zeros(0, dtype=torch.int32, device="cuda"))
    res = scorer.result()
    assert res.rows.tolist() == [0, 0] and res.loss.tolist() == [0.0, 0.0] and not res.confusion_matrix.any() and scorer._work is None


def test_a_captured_add_replayed_on_new_scores_tallies_the_new_scores():
    case = next(c for c in CASES if c["name"] == "grid-C33-N257-mode1")
    scores, labels, groups, want = built(case)
    K, N, C = scores.shape
    rng = np.random.default_rng(5)
    others = [np.ascontiguousarray(scores[:, rng.permutation(N)]) for _ in range(2)]
    scorer = scoring.Scorer(K, C, 1, n_groups=case["n_groups"])
    d_scores, d_labels = torch.from_numpy(scores).cuda(), torch.from_numpy(labels).cuda()
    d_groups = torch.from_numpy(groups).cuda() if groups is not None else None
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        scorer.add(d_scores, d_labels, d_groups)                      # warm-up: the workspace is sized outside the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    scorer.reset()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        scorer.add(d_scores, d_labels, d_groups)
    assert not scorer.raw().tally.any()                               # capturing ran nothing
    total = None
    for other in others:
        d_scores.copy_(torch.from_numpy(other).cuda())
        graph.replay()
        w = sc.host(case, other, labels, groups)
        total = w if total is None else SimpleNamespace(tally=total.tally + w.tally, confusion=total.confusion + w.confusion,
                                                                group_tally=total.group_tally + w.group_tally)
    torch.cuda.synchronize()
    assert_integers(scorer.raw(), total)


def test_reset_and_result():
    case = next(c for c in CASES if c["name"] == "grid-C7-N257-mode0")
    scores, labels, groups, want = built(case)
    K, N, C = scores.shape
    scorer = scoring.Scorer(K, C, 0, n_groups=case["n_groups"])
    args = [torch.from_numpy(scores).cuda(), torch.from_numpy(labels).to(torch.int64).cuda()] + ([torch.from_numpy(groups).cuda()] if groups is not None else [])
    scorer.add(*args)
    scorer.add(*args)
    res = scorer.result()
    assert res.rows.tolist() == (2 * want.tally[:, 0]).tolist() and np.array_equal(res.confusion_matrix, 2 * want.confusion)
    assert res.confusion_matrix.dtype == np.int64 and res.ignored.tolist() == (2 * want.tally[:, 2]).tolist()
    scorer.reset()
    scorer.add(args[0].transpose(0, 1).contiguous().transpose(0, 1), *args[1:])          # a strided view of the same values
    res = scorer.result()
    assert res.rows.tolist() == want.tally[:, 0].tolist() and np.array_equal(res.accuracy, want.tally[:, 1] / want.tally[:, 0])
    assert np.allclose(res.loss, want.loss_sum / want.tally[:, 0], rtol=1e-12, atol=0)
    if case["n_groups"]:
        assert np.array_equal(res.group_rows, want.group_tally[:, :, 0])
    for bad in (dict(row_loss=torch.zeros((K, N), device="cuda")), dict(pred=torch.zeros((K, N), dtype=torch.int64, device="cuda")),
                dict(pred=torch.zeros((K, N + 1), dtype=torch.int32, device="cuda"))):
        with pytest.raises(ValueError, match="row_loss|pred"):
            scorer.add(*args, **bad)


def test_invalid_labels_raise_in_result_with_the_model_index():
    scorer = scoring.Scorer(3, 4, 0, n_groups=2)
    probs = torch.full((3, 6, 4), 0.25, device="cuda")
    labels = torch.zeros((3, 6), dtype=torch.int32, device="cuda")
    labels[1, 2], labels[1, 4], labels[2, 0] = 4, -5, 1 << 30
    pred = torch.full((3, 6), -7, dtype=torch.int32, device="cuda")
    scorer.add(probs, labels, torch.tensor([0, 1, 0, 1, 0, 1], device="cuda"), pred=pred)
    with pytest.raises(RuntimeError, match=r"model 1: 2 rows"):
        scorer.result()
    raw = scorer.raw()
    assert raw.tally.tolist() == [[6, 6, 0, 0], [4, 4, 0, 2], [5, 5, 0, 1]] and not pred.cpu().numpy().any()
    scorer.reset()
    scorer.add(probs, labels.clamp(0, 3), torch.tensor([0, 1, 2, 1, 0, -1], device="cuda"))
    with pytest.raises(RuntimeError, match=r"model 0: 2 rows"):
        scorer.result()
