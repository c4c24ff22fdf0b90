"""mkws_detect_live_step_routes: R live detectors of one head each, route r following the pushes of ITS SLOT with thresholds of its own, in
one launch.  Every route is held byte for byte to mkws_detect_stream (detect_on_device) over the rows it received since it was attached
and, state slice by state slice, to mkws_detect_live_step with one head."""
import functools

import numpy as np
import pytest

from multilingual_kws_amd import _lib, detector
from tests.util_live import SETTINGS, THRESHOLDS, WINDOWS, push_plan, scripted_probs, times_ms

pytestmark = pytest.mark.gpu
S, R = 3, 7
ROUTE_SLOT = (0, 0, 1, -1, 2, 1, 2)                                        # two routes on slot 0; route 3 disabled; route 5 attached later
LATE, ATTACH_TICK = 5, 40
ROLLS = (0, 55, 131, 7, 99, 13, 170)                                       # route r hears the script rolled by ROLLS[r] windows
ENABLED = [r for r in range(R) if ROUTE_SLOT[r] >= 0]
PATTERN = 0x5A5A5A5A5A5A5A5A                                               # what untouched state words hold
SPARE = 3                                                                  # words between two state slices: the stride is wider than a block


def _thresholds(n_thr):
    """float64 [R, n_thr]: every route its own row (the two routes of slot 0 differ)."""
    if n_thr == 1:
        return np.asarray([[THRESHOLDS[r % 4]] for r in range(R)], np.float64)
    return np.asarray([np.roll(THRESHOLDS, r) for r in range(R)], np.float64)


def _plans(h):
    """Per slot its [(first window, count)] per tick, all of the same length: slot 0 one leading empty tick, slot 1 an empty tick after
    every third push, slot 2 four leading empty ticks and one after every seventh push; then empty ticks until the slowest is through."""
    plans = [push_plan(WINDOWS, h, leading_empty=1), [], [(0, 0)] * 4]
    for i, (first, count) in enumerate(push_plan(WINDOWS, h)):
        plans[1] += [(first, count)] + ([(first + count, 0)] if i % 3 == 2 else [])
        plans[2] += [(first, count)] + ([(first + count, 0)] if i % 7 == 6 else [])
    ticks = max(len(p) for p in plans)
    return [p + [(WINDOWS, 0)] * (ticks - len(p)) for p in plans]


def _since(plans, r):
    """The first window of its slot that route r hears."""
    return plans[ROUTE_SLOT[r]][ATTACH_TICK][0] if r == LATE else 0


@functools.lru_cache(maxsize=None)
def _plane(r, nan_rows=()):
    """Route r's probability rows [WINDOWS, 3], indexed by its slot's windows (computed once, shared, not modified)."""
    p = np.roll(scripted_probs((0,))[0], ROLLS[r], axis=0)
    for w in nan_rows:
        p[w] = np.nan
    return p


@functools.lru_cache(maxsize=None)
def _whole(setting, fired_only, n_thr, r, since, nan_rows=()):
    """detect_on_device over what route r hears: its rows from window `since` on, at its slot's window times, its own thresholds."""
    avg, sup, minc = setting
    return detector.detect_on_device(_plane(r, nan_rows)[None, since:], times_ms()[since:], _thresholds(n_thr)[r], avg, sup, minc, trace=True,
                                     fired_only=bool(fired_only))


def _run_routes(planes, plans, h, setting, fired_only, n_thr):
    """The ticks of `plans` through detect_live_step_routes without a synchronisation in between (but one look at the late route's state
    before it is attached) -> per route (records per threshold, total counts [T], scores [windows heard]), and what the one-stream check needs."""
    import torch
    avg, sup, minc = setting
    times, T = times_ms(), n_thr
    history = detector.live_history(avg, 320, 16000)
    ticks = len(plans[0])
    assert ticks > ATTACH_TICK + 1
    h_probs, h_meta = np.full((ticks, R * h, 3), 0.99, np.float32), np.full((ticks, S, 2 + h), -12345, np.int64)   # rows past count must not be read
    for s in range(S):
        for i, (first, count) in enumerate(plans[s]):
            h_meta[i, s, :2] = count, first
            h_meta[i, s, 2:2 + count] = times[first:first + count]
    for r in ENABLED:
        for i, (first, count) in enumerate(plans[ROUTE_SLOT[r]]):
            h_probs[i, r * h:r * h + count] = planes[r][first:first + count]
    d_probs, d_meta = torch.from_numpy(h_probs).cuda(), torch.from_numpy(h_meta).cuda()
    d_thr = torch.from_numpy(_thresholds(T)).cuda()
    d_slot = torch.tensor([-1 if r == LATE else s for r, s in enumerate(ROUTE_SLOT)], dtype=torch.int32, device="cuda")
    words = detector.live_detector_state_routes(1, T, history).shape[1]
    wide = torch.full((R, words + SPARE), PATTERN, dtype=torch.int64, device="cuda")
    states = wide[:, :words]
    for r in ENABLED:
        if r != LATE:
            states[r].zero_()
    d_out = torch.full((ticks, detector.live_out_words_routes(R, T, h)), -1, dtype=torch.int64, device="cuda")
    d_scores = torch.full((ticks, R, h), -7.0, dtype=torch.float64, device="cuda")
    for i in range(ticks):
        if i == ATTACH_TICK:
            assert bool((wide[LATE] == PATTERN).all().cpu()), "a route that is not attached had its state written"
            states[LATE].zero_()                                           # attach: a fresh detector, then the table entry
            d_slot[LATE] = ROUTE_SLOT[LATE]
        detector.detect_live_step_routes(states, d_probs[i], d_meta[i], d_slot, d_thr, avg, sup, minc, history, fired_only=fired_only, out=d_out[i],
                                         scores=d_scores[i])
    out, scores = d_out.cpu().numpy(), d_scores.cpu().numpy()
    unpacked = [detector.live_unpack_many(out[i], R, 1, T, h) for i in range(ticks)]
    results = {}
    for r in range(R):
        slot = ROUTE_SLOT[r]
        heard = [(i, first, count) for i, (first, count) in enumerate(plans[slot])] if slot >= 0 else []
        if r == LATE:
            heard = [x for x in heard if x[0] >= ATTACH_TICK]
        on = {i for i, _, _ in heard}
        for i in range(ticks):
            if i not in on:                                                # disabled (or not yet attached): zero counts, scores untouched
                assert not unpacked[i][0][r].any() and (scores[i, r] == -7.0).all(), (r, i)
        records, total = [[] for _ in range(T)], np.zeros(T, np.int64)
        for i, first, count in heard:
            counts, events = unpacked[i][0][r, 0], unpacked[i][1][r, 0]
            assert counts.min() >= 0 and counts.max() <= count
            assert (scores[i, r, count:] == -7.0).all()                    # scores past count are left untouched
            total += counts
            for k in range(T):
                ev = events[k, :counts[k]].copy()
                ev["window"] += first
                records[k].append(ev)
        results[r] = ([np.concatenate(x) if x else np.zeros(0, detector.EVENT_DTYPE) for x in records], total,
                      np.concatenate([scores[i, r, :c] for i, _, c in heard]) if heard else np.zeros(0))
    return results, wide, (d_probs, d_meta, d_thr, history, words)


def _assert_equals_whole(result, want, since, T):
    records, total, scores = result
    for k in range(T):
        ev = want.event_buffer[0, k, :want.counts[0, k]].copy()
        ev["window"] += since                                              # detect_on_device counts from the first row it was given
        assert records[k].tobytes() == ev.tobytes(), k
        assert total[k] == len(ev)
    assert scores.tobytes() == np.ascontiguousarray(want.scores[0]).tobytes()


@pytest.mark.parametrize("fired_only", [0, 1])
@pytest.mark.parametrize("n_thr", [1, 4])
@pytest.mark.parametrize("h", [1, 3, 7])
@pytest.mark.parametrize("setting", SETTINGS)
def test_every_route_equals_the_stateless_detector_and_the_one_head_step(setting, h, n_thr, fired_only):
    import torch
    plans = _plans(h)
    assert len({tuple(p) for p in plans}) == S and all(sum(c for _, c in p) == WINDOWS for p in plans)
    assert any(c == 0 for _, c in plans[1][1:-1]) and plans[2][:4] == [(0, 0)] * 4 and plans[0][0] == (0, 0)
    assert 0 < _since(plans, LATE) < WINDOWS - 20 and _thresholds(n_thr)[0].tolist() != _thresholds(n_thr)[1].tolist()
    results, wide, (d_probs, d_meta, d_thr, history, words) = _run_routes([_plane(r) for r in range(R)], plans, h, setting, fired_only, n_thr)
    for r in ENABLED:
        want = _whole(setting, fired_only, n_thr, r, _since(plans, r))
        assert all(int(want.events[0][k]["fired"].sum()) >= 1 for k in range(n_thr)), "every enabled route must fire in every lane"
        _assert_equals_whole(results[r], want, _since(plans, r), n_thr)
        assert all(int(results[r][0][k]["fired"].sum()) >= 1 for k in range(n_thr))
    # the two routes of slot 0 heard the same pushes and report events of their own
    assert any(results[0][0][k].tobytes() != results[1][0][k].tobytes() for k in range(n_thr))
    # the disabled route and the words between the slices
    assert bool((wide[3] == PATTERN).all().cpu()) and bool((wide[:, words:] == PATTERN).all().cpu())
    assert not results[3][1].any() and results[3][2].size == 0
    # every slice is the block the one-stream, one-head step leaves after the same pushes
    avg, sup, minc = setting
    for r in ENABLED:
        one = detector.live_detector_state(1, n_thr, history)
        assert one.numel() == words
        mine = d_probs[:, r * h:(r + 1) * h].contiguous()
        heard = 0
        for i in range(ATTACH_TICK if r == LATE else 0, len(plans[0])):
            detector.detect_live_step(one, mine[i][None], d_meta[i, ROUTE_SLOT[r]], d_thr[r], avg, sup, minc, history, fired_only=fired_only)
            heard += plans[ROUTE_SLOT[r]][i][1]
        assert torch.equal(wide[r, :words], one), r
        assert int(one[0].cpu()) == heard == WINDOWS - _since(plans, r)


def test_a_nan_row_silences_only_its_own_route():
    """Routes 0 and 1 listen to the same slot; route 1's probabilities have NaN rows."""
    setting, h, T, nan_rows = SETTINGS[0], 7, 4, (100, 101, 102, 150)
    plans = _plans(h)
    planes = [_plane(r, nan_rows if r == 1 else ()) for r in range(R)]
    results, _, _ = _run_routes(planes, plans, h, setting, 0, T)
    for r in ENABLED:
        want = _whole(setting, 0, T, r, _since(plans, r), nan_rows if r == 1 else ())
        _assert_equals_whole(results[r], want, _since(plans, r), T)
    assert np.isnan(results[1][2][100:108]).all() and all(not np.isnan(results[r][2]).any() for r in ENABLED if r != 1)
    clean, dirty = _whole(setting, 0, T, 1, 0), _whole(setting, 0, T, 1, 0, nan_rows)
    assert dirty.counts.sum() < clean.counts.sum() or dirty.event_buffer.tobytes() != clean.event_buffer.tobytes()


def test_live_step_routes_refuses_what_it_documents():
    import torch
    h, history, T = 2, 6, len(THRESHOLDS)
    states = detector.live_detector_state_routes(R, T, history)
    need = _lib.lib().mkws_detect_live_state_bytes(1, T, history)
    assert 8 * states.shape[1] == need
    probs = torch.zeros((R * h, 3), dtype=torch.float32, device="cuda")
    meta = torch.zeros((S, 2 + h), dtype=torch.int64, device="cuda")
    d_thr = torch.from_numpy(_thresholds(T)).cuda()
    d_slot = torch.tensor(ROUTE_SLOT, dtype=torch.int32, device="cuda")
    out = torch.zeros(detector.live_out_words_routes(R, T, h), dtype=torch.int64, device="cuda")
    L = _lib.lib()

    def step(state_ptr=states.data_ptr(), stride=need, n=R, slot_ptr=d_slot.data_ptr(), n_slots=S, max_new=h, classes=3, target=2, n_thr=T, avg=100.0,
             sup=500.0, history=history, counts=out.data_ptr()):
        return L.mkws_detect_live_step_routes(state_ptr, stride, n, slot_ptr, n_slots, probs.data_ptr(), meta.data_ptr(), max_new, classes, target,
                                              d_thr.data_ptr(), n_thr, avg, sup, 4, 0, history, out.data_ptr() + 8 * ((R * T + 1) // 2), counts, None, None)
    assert step() == 0
    assert step(history=detector.LIVE_MAX_HISTORY + 1) == -2 and step(n_thr=1025) == -2 and step(max_new=detector.LIVE_MAX_NEW + 1) == -2
    for bad in (dict(stride=0), dict(stride=need - 8), dict(stride=need + 4), dict(n=-1), dict(state_ptr=None), dict(counts=None), dict(slot_ptr=None),
                dict(n_slots=-1), dict(max_new=-1), dict(n_thr=0), dict(target=3), dict(target=-1), dict(classes=0), dict(avg=-1.0), dict(avg=float("nan")),
                dict(sup=float("nan")), dict(history=0)):
        assert step(**bad) == -1, bad
    assert step(n=0) == 0 and step(max_new=0) == 0 and step(stride=need + 64) == 0
    assert step(n_slots=0) == 0                                            # no slot: every route is outside [0, 0), zero counts
    torch.cuda.synchronize()
    assert not detector.live_unpack_routes(out.cpu().numpy(), R, T, h)[0].any() and not bool(states.any().cpu())
    with pytest.raises(_lib.MkwsError) as ei:
        detector.detect_live_step_routes(states, probs, meta, d_slot, d_thr, 100, 500, 4, detector.LIVE_MAX_HISTORY + 1, out=out)
    assert ei.value.code == -2
    with pytest.raises(ValueError):
        detector.detect_live_step_routes(states, probs[:h].contiguous(), meta, d_slot, d_thr, 100, 500, 4, history, out=out)
    with pytest.raises(ValueError):
        detector.detect_live_step_routes(states, probs, meta, d_slot, d_thr, 100, 500, 4, history, out=out[:-1])
    with pytest.raises(ValueError):
        detector.detect_live_step_routes(states, probs, meta, d_slot[:-1], d_thr, 100, 500, 4, history, out=out)
    torch.cuda.synchronize()
