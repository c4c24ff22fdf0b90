"""mkws_detect_live_step: the detector fed push by push, held byte for byte to mkws_detect_stream (detect_on_device) over the whole
stream -- whose own yardstick is the host class -- and to the host restatement LiveDetectorHost directly."""
import functools

import numpy as np
import pytest

from multilingual_kws_amd import _lib, detector
from tests.util_live import SETTINGS, THRESHOLDS, WINDOWS, lane_reference, push_plan, scripted_probs, times_ms

pytestmark = pytest.mark.gpu
N, T = 3, len(THRESHOLDS)


@functools.lru_cache(maxsize=None)
def _whole(setting, fired_only, nan_rows=()):
    """detect_on_device over the whole scripted stream (computed once per case, shared, not modified)."""
    probs = scripted_probs()
    for w in nan_rows:
        probs[1, w] = np.nan
    avg, sup, minc = setting
    return probs, detector.detect_on_device(probs, times_ms(), THRESHOLDS, avg, sup, minc, trace=True, fired_only=bool(fired_only))


def _run_live(probs, times, plan, h, setting, fired_only, state=None, history=None):
    """The pushes of `plan` through detect_live_step without a synchronisation in between -> (per lane the concatenated
    (window + base, fired, score) records, total counts [N, T], scores [N, windows of the plan], the state block)."""
    import torch
    avg, sup, minc = setting
    history = history or detector.live_history(avg, 320, 16000)
    if state is None:
        state = detector.live_detector_state(N, T, history)
    P = len(plan)
    h_probs, h_meta = np.zeros((P, N, h, 3), np.float32), np.zeros((P, 2 + h), np.int64)
    for i, (first, count) in enumerate(plan):
        h_probs[i, :, :count] = probs[:, first:first + count]
        h_probs[i, :, count:] = 0.99                                       # rows past count must not be read
        h_meta[i, :2] = count, first
        h_meta[i, 2:2 + count] = times[first:first + count]
        h_meta[i, 2 + count:] = -12345
    d_probs, d_meta = torch.from_numpy(h_probs).cuda(), torch.from_numpy(h_meta).cuda()
    d_thr = torch.tensor(THRESHOLDS, dtype=torch.float64, device="cuda")
    words = detector.live_out_words(N, T, h)
    d_out = torch.full((P, words), -1, dtype=torch.int64, device="cuda")
    d_scores = torch.full((P, N, h), -7.0, dtype=torch.float64, device="cuda")
    for i in range(P):
        detector.detect_live_step(state, d_probs[i], d_meta[i], d_thr, avg, sup, minc, history, fired_only=fired_only, out=d_out[i], scores=d_scores[i])
    out, scores = d_out.cpu().numpy(), d_scores.cpu().numpy()
    records = [[[] for _ in range(T)] for _ in range(N)]
    total = np.zeros((N, T), np.int64)
    for i, (first, count) in enumerate(plan):
        counts, events = detector.live_unpack(out[i], N, T, h)
        assert counts.min() >= 0 and counts.max() <= count
        total += counts
        for n in range(N):
            for k in range(T):
                ev = events[n, k, :counts[n, k]].copy()
                ev["window"] += first
                records[n][k].append(ev)
    records = [[np.concatenate(r) for r in row] for row in records]
    return records, total, np.concatenate([scores[i, :, :c] for i, (_, c) in enumerate(plan)], axis=1), state


def _assert_equals_whole(records, total, scores, want, upto=WINDOWS):
    for n in range(N):
        for k in range(T):
            ev = want.event_buffer[n, k, :want.counts[n, k]]
            ev = ev[ev["window"] < upto]
            assert records[n][k].tobytes() == ev.tobytes(), (n, k)
            assert total[n, k] == len(ev)
    assert scores.tobytes() == np.ascontiguousarray(want.scores[:, :upto]).tobytes()


@pytest.mark.parametrize("fired_only", [0, 1])
@pytest.mark.parametrize("h", [1, 3, 7])
@pytest.mark.parametrize("setting", SETTINGS)
def test_live_steps_concatenate_to_the_stateless_detector(setting, h, fired_only):
    probs, want = _whole(setting, fired_only)
    assert all(int(want.events[n][k]["fired"].sum()) >= 3 for n in range(N) for k in range(T)), "the scripted stream must fire in every lane"
    records, total, scores, _ = _run_live(probs, times_ms(), push_plan(WINDOWS, h, leading_empty=1), h, setting, fired_only)
    _assert_equals_whole(records, total, scores, want)


def test_live_step_against_the_host_class_directly():
    setting, h = SETTINGS[0], 3
    probs, times = scripted_probs(), times_ms()
    records, total, scores, _ = _run_live(probs, times, push_plan(WINDOWS, h), h, setting, 0)
    host = detector.LiveDetectorHost(N, THRESHOLDS, *setting)
    want = [[[] for _ in range(T)] for _ in range(N)]
    for first, count in push_plan(WINDOWS, h):
        _, events, _ = host.step(probs[:, first:first + count], times[first:first + count])
        for n in range(N):
            for k in range(T):
                want[n][k] += [(first + w, f, s) for w, f, s in events[n][k].tolist()]
    assert [[r.tolist() for r in row] for row in records] == want
    assert records[2][1].tolist() == lane_reference(probs[2], times, THRESHOLDS[1], *setting) and total[2, 1] >= 3


def test_one_step_of_more_windows_than_the_workgroup_has_threads():
    """max_new = 300 with four thresholds (a 64-thread workgroup): the whole stream in one step, then as 300-window steps of a longer one."""
    setting = SETTINGS[0]
    probs, want = _whole(setting, 0)
    records, total, scores, _ = _run_live(probs, times_ms(), [(0, 0), (0, WINDOWS)], 300, setting, 0)
    _assert_equals_whole(records, total, scores, want)


def test_empty_push_changes_nothing_and_a_zeroed_state_is_a_fresh_stream():
    import torch
    setting, h = SETTINGS[0], 3
    probs, want = _whole(setting, 0)
    times = times_ms()
    first_100 = push_plan(100, h)
    _, _, _, state = _run_live(probs, times, first_100, h, setting, 0)
    before = state.clone()
    records, total, _, state = _run_live(probs, times, [(100, 0)], h, setting, 0, state=state)
    assert torch.equal(state, before) and total.sum() == 0 and all(len(r) == 0 for row in records for r in row)
    assert int(state.view(torch.int64)[0].cpu()) == 100                     # windows seen by head 0
    state.zero_()                                                           # reset is a memset
    records, total, scores, _ = _run_live(probs, times, push_plan(60, h), h, setting, 0, state=state)
    _assert_equals_whole(records, total, scores, want, upto=60)


def test_nan_rows_give_the_stateless_kernels_result():
    setting, h = SETTINGS[0], 7
    nan_rows = (100, 101, 102, 150)
    probs, want = _whole(setting, 0, nan_rows)
    assert np.isnan(want.scores[1, 100:108]).all() and not np.isnan(want.scores[0]).any()
    records, total, scores, _ = _run_live(probs, times_ms(), push_plan(WINDOWS, h), h, setting, 0)
    _assert_equals_whole(records, total, scores, want)


def test_live_step_refuses_what_it_documents():
    import torch
    with pytest.raises(ValueError):
        detector.live_detector_state(N, T, detector.LIVE_MAX_HISTORY + 1)
    state = detector.live_detector_state(N, T, 6)
    probs = torch.zeros((N, 2, 3), dtype=torch.float32, device="cuda")
    meta = torch.zeros(4, dtype=torch.int64, device="cuda")
    d_thr = torch.tensor(THRESHOLDS, dtype=torch.float64, device="cuda")
    out = torch.zeros(detector.live_out_words(N, T, 2), dtype=torch.int64, device="cuda")
    L = _lib.lib()

    def step(state_ptr=state.data_ptr(), max_new=2, n_heads=N, classes=3, target=2, n_thr=T, avg=100.0, sup=500.0, history=6, counts=out.data_ptr()):
        return L.mkws_detect_live_step(state_ptr, probs.data_ptr(), meta.data_ptr(), max_new, n_heads, classes, target, d_thr.data_ptr(), n_thr, avg, sup,
                                       4, 0, history, out.data_ptr() + 8 * ((N * T + 1) // 2), counts, None, None)
    assert step() == 0
    assert step(history=detector.LIVE_MAX_HISTORY + 1) == -2 and step(n_thr=1025) == -2 and step(max_new=detector.LIVE_MAX_NEW + 1) == -2
    for bad in (dict(state_ptr=None), dict(counts=None), dict(n_heads=-1), dict(max_new=-1), dict(n_thr=0), dict(target=3), dict(target=-1),
                dict(classes=0), dict(avg=-1.0), dict(avg=float("nan")), dict(sup=float("nan")), dict(history=0)):
        assert step(**bad) == -1, bad
    assert step(n_heads=0) == 0 and step(max_new=0) == 0
    with pytest.raises(_lib.MkwsError) as ei:
        detector.detect_live_step(state, probs, meta, d_thr, 100, 500, 4, detector.LIVE_MAX_HISTORY + 1, out=out)
    assert ei.value.code == -2
    torch.cuda.synchronize()
