"""mkws_detect_live_step_many: S live detectors stepped in one launch, every stream on a schedule of its own, held byte for byte to
mkws_detect_stream (detect_on_device) over each whole stream and, state slice by state slice, to mkws_detect_live_step."""
import functools

import numpy as np
import pytest

from multilingual_kws_amd import _lib, detector
from tests.util_live import SETTINGS, THRESHOLDS, WINDOWS, push_plan, scripted_probs, times_ms

pytestmark = pytest.mark.gpu
S, N, T = 3, 3, len(THRESHOLDS)
ROLLS = (0, 55, 131)                                                       # stream s = the script rolled by ROLLS[s] windows


@functools.lru_cache(maxsize=None)
def _whole(setting, fired_only, s, nan_rows=()):
    """Stream s and detect_on_device over all of it (computed once per case, shared, not modified)."""
    probs = np.roll(scripted_probs(), ROLLS[s], axis=1)
    for w in nan_rows:
        probs[1, w] = np.nan
    avg, sup, minc = setting
    return probs, detector.detect_on_device(probs, times_ms(), THRESHOLDS, avg, sup, minc, trace=True, fired_only=bool(fired_only))


def _plans(h):
    """Per stream its [(first window, count)] per tick, all of the same length: stream 0 one leading empty tick, stream 1 an empty tick after
    every third push, stream 2 four leading empty ticks and one after every seventh push; then empty ticks until the slowest is through."""
    plans = [push_plan(WINDOWS, h, leading_empty=1), [], [(0, 0)] * 4]
    for i, (first, count) in enumerate(push_plan(WINDOWS, h)):
        plans[1] += [(first, count)] + ([(first + count, 0)] if i % 3 == 2 else [])
        plans[2] += [(first, count)] + ([(first + count, 0)] if i % 7 == 6 else [])
    ticks = max(len(p) for p in plans)
    return [p + [(WINDOWS, 0)] * (ticks - len(p)) for p in plans]


def _run_many(streams, plans, h, setting, fired_only):
    """The ticks of `plans` through detect_live_step_many without a synchronisation in between -> per stream (records per lane, total counts
    [N, T], scores [N, windows]) and the state tensor."""
    import torch
    avg, sup, minc = setting
    times = times_ms()
    history = detector.live_history(avg, 320, 16000)
    ticks = len(plans[0])
    h_probs, h_meta = np.full((ticks, N, S * h, 3), 0.99, np.float32), np.full((ticks, S, 2 + h), -12345, np.int64)   # rows past count must not be read
    for s in range(S):
        for i, (first, count) in enumerate(plans[s]):
            h_probs[i, :, s * h:s * h + count] = streams[s][:, first:first + count]
            h_meta[i, s, :2] = count, first
            h_meta[i, s, 2:2 + count] = times[first:first + count]
    d_probs, d_meta = torch.from_numpy(h_probs).cuda(), torch.from_numpy(h_meta).cuda()
    d_thr = torch.tensor(THRESHOLDS, dtype=torch.float64, device="cuda")
    states = detector.live_detector_state_many(S, N, T, history)
    d_out = torch.full((ticks, detector.live_out_words_many(S, N, T, h)), -1, dtype=torch.int64, device="cuda")
    d_scores = torch.full((ticks, S, N, h), -7.0, dtype=torch.float64, device="cuda")
    for i in range(ticks):
        detector.detect_live_step_many(states, d_probs[i], d_meta[i], d_thr, avg, sup, minc, history, fired_only=fired_only, out=d_out[i], scores=d_scores[i])
    out, scores = d_out.cpu().numpy(), d_scores.cpu().numpy()
    unpacked = [detector.live_unpack_many(out[i], S, N, T, h) for i in range(ticks)]
    results = []
    for s in range(S):
        records, total = [[[] for _ in range(T)] for _ in range(N)], np.zeros((N, T), np.int64)
        for i, (first, count) in enumerate(plans[s]):
            counts, events = unpacked[i][0][s], unpacked[i][1][s]
            assert counts.min() >= 0 and counts.max() <= count
            assert (scores[i, s, :, count:] == -7.0).all()                 # scores past count are left untouched
            total += counts
            for n in range(N):
                for k in range(T):
                    ev = events[n, k, :counts[n, k]].copy()
                    ev["window"] += first
                    records[n][k].append(ev)
        records = [[np.concatenate(r) for r in row] for row in records]
        results.append((records, total, np.concatenate([scores[i, s, :, :c] for i, (_, c) in enumerate(plans[s])], axis=1)))
    return results, states, (d_probs, d_meta, d_thr, history)


def _assert_equals_whole(result, want):
    records, total, scores = result
    for n in range(N):
        for k in range(T):
            ev = want.event_buffer[n, k, :want.counts[n, k]]
            assert records[n][k].tobytes() == ev.tobytes(), (n, k)
            assert total[n, k] == len(ev)
    assert scores.tobytes() == np.ascontiguousarray(want.scores).tobytes()


@pytest.mark.parametrize("fired_only", [0, 1])
@pytest.mark.parametrize("h", [1, 3, 7])
@pytest.mark.parametrize("setting", SETTINGS)
def test_many_streams_equal_the_stateless_detector_and_the_one_stream_step(setting, h, fired_only):
    import torch
    wholes = [_whole(setting, fired_only, s) for s in range(S)]
    for _, want in wholes:
        assert all(int(want.events[n][k]["fired"].sum()) >= 3 for n in range(N) for k in range(T)), "every stream must fire in every lane"
    plans = _plans(h)
    assert len({tuple(p) for p in plans}) == S and all(sum(c for _, c in p) == WINDOWS for p in plans)
    assert any(c == 0 for _, c in plans[1][1:-1]) and plans[2][:4] == [(0, 0)] * 4
    results, states, (d_probs, d_meta, d_thr, history) = _run_many([w[0] for w in wholes], plans, h, setting, fired_only)
    for s in range(S):
        _assert_equals_whole(results[s], wholes[s][1])
    # every slice is the block the one-stream step leaves after the same pushes (its rows of the same buffers, copied out)
    avg, sup, minc = setting
    for s in range(S):
        one = detector.live_detector_state(N, T, history)
        assert one.numel() == states.shape[1]
        mine = d_probs[:, :, s * h:(s + 1) * h].contiguous()
        for i in range(len(plans[s])):
            detector.detect_live_step(one, mine[i], d_meta[i, s], d_thr, avg, sup, minc, history, fired_only=fired_only)
        assert torch.equal(states[s], one), s
        assert int(one[0].cpu()) == WINDOWS


def test_a_nan_row_silences_only_its_own_stream():
    setting, h, nan_rows = SETTINGS[0], 7, (100, 101, 102, 150)
    wholes = [_whole(setting, 0, s, nan_rows if s == 1 else ()) for s in range(S)]
    assert np.isnan(wholes[1][1].scores[1, 100:108]).all() and not np.isnan(wholes[1][1].scores[0]).any()
    results, _, _ = _run_many([w[0] for w in wholes], _plans(h), h, setting, 0)
    for s in range(S):
        _assert_equals_whole(results[s], wholes[s][1])
    assert not np.isnan(results[0][2]).any() and not np.isnan(results[2][2]).any() and np.isnan(results[1][2][1]).any()
    clean = _whole(setting, 0, 1)[1]
    assert wholes[1][1].counts[1].sum() < clean.counts[1].sum() or wholes[1][1].event_buffer.tobytes() != clean.event_buffer.tobytes()


def test_live_step_many_refuses_what_it_documents():
    import torch
    h, history = 2, 6
    states = detector.live_detector_state_many(S, N, T, history)
    need = _lib.lib().mkws_detect_live_state_bytes(N, T, history)
    assert 8 * states.shape[1] == need
    probs = torch.zeros((N, S * h, 3), dtype=torch.float32, device="cuda")
    meta = torch.zeros((S, 2 + h), dtype=torch.int64, device="cuda")
    d_thr = torch.tensor(THRESHOLDS, dtype=torch.float64, device="cuda")
    out = torch.zeros(detector.live_out_words_many(S, N, T, h), dtype=torch.int64, device="cuda")
    L = _lib.lib()

    def step(state_ptr=states.data_ptr(), stride=need, n=S, max_new=h, n_heads=N, classes=3, target=2, n_thr=T, avg=100.0, sup=500.0, history=history,
             counts=out.data_ptr()):
        return L.mkws_detect_live_step_many(state_ptr, stride, n, probs.data_ptr(), meta.data_ptr(), max_new, n_heads, classes, target, d_thr.data_ptr(),
                                            n_thr, avg, sup, 4, 0, history, out.data_ptr() + 8 * ((S * N * T + 1) // 2), counts, None, None)
    assert step() == 0
    assert step(history=detector.LIVE_MAX_HISTORY + 1) == -2 and step(n_thr=1025) == -2 and step(max_new=detector.LIVE_MAX_NEW + 1) == -2
    for bad in (dict(stride=0), dict(stride=need - 8), dict(stride=need + 4), dict(n=-1), dict(state_ptr=None), dict(counts=None), dict(n_heads=-1),
                dict(max_new=-1), dict(n_thr=0), dict(target=3), dict(target=-1), dict(classes=0), dict(avg=-1.0), dict(avg=float("nan")),
                dict(sup=float("nan")), dict(history=0)):
        assert step(**bad) == -1, bad
    assert step(n=0) == 0 and step(n_heads=0) == 0 and step(max_new=0) == 0 and step(stride=need + 64) == 0
    with pytest.raises(_lib.MkwsError) as ei:
        detector.detect_live_step_many(states, probs, meta, d_thr, 100, 500, 4, detector.LIVE_MAX_HISTORY + 1, out=out)
    assert ei.value.code == -2
    with pytest.raises(ValueError):
        detector.detect_live_step_many(states, probs[:, :h].contiguous(), meta, d_thr, 100, 500, 4, history, out=out)
    with pytest.raises(ValueError):
        detector.detect_live_step_many(states, probs, meta, d_thr, 100, 500, 4, history, out=out[:-1])
    torch.cuda.synchronize()
