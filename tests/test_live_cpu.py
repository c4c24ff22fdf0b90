"""The host side of the live session (LiveSession, mkws_frontend_live_push_f32, mkws_detect_live_step): geometry, the host restatement of
the live detector, the re-buffering of chunks into pushes and the history rule.  No GPU."""
import numpy as np
import pytest

from multilingual_kws_amd import _lib, detector, frontend
from multilingual_kws_amd.embedding import batch_streaming_analysis as bsa
from tests.util_live import SETTINGS, THRESHOLDS, lane_reference, push_plan, scripted_probs, times_ms

CLIP, HOP, RATE = 16000, 320, 16000


@pytest.mark.parametrize("n", [15999, 16000, 16319, 16320, 25600])
def test_live_geometry_against_the_offline_window_list(n):
    """A live stream cannot know that it has ended, so it emits the window its last sample completes: W(n) = 1 + (n - clip) // hop.  The
    reference's range(0, n - clip, hop) leaves exactly that window out when n - clip is a multiple of the hop -- W(n) is its list for one
    more sample -- and the two agree on where every window starts and on its time."""
    W = frontend.live_windows(n, CLIP, HOP)
    offline = bsa.window_offsets(n, CLIP, HOP)
    assert W == len(bsa.window_offsets(n + 1, CLIP, HOP))
    assert len(offline) == W - (1 if n >= CLIP and (n - CLIP) % HOP == 0 else 0)
    assert {15999: 0, 16000: 1, 16319: 1, 16320: 2, 25600: 31}[n] == W
    flags = bsa.default_live_flags([0.5])
    _, stride, offsets = bsa._stream_windows(np.zeros((1, W, 3), np.float32), flags, RATE, n + 1)
    assert stride == HOP and offsets == [w * HOP for w in range(W)] and offsets[:len(offline)] == offline
    assert [frontend.live_window_time_ms(w, HOP, RATE) for w in range(W)] == [int(off * 1000 / RATE) for off in offsets]
    # push by push: the counts add up to W(n), whatever the push size
    for h in (1, 4):
        seen, total = 0, 0
        while seen + h * HOP <= n:
            total += frontend.live_windows(seen + h * HOP, CLIP, HOP) - frontend.live_windows(seen, CLIP, HOP)
            seen += h * HOP
        assert total == frontend.live_windows(seen, CLIP, HOP) <= W


@pytest.mark.parametrize("setting", SETTINGS)
@pytest.mark.parametrize("h", [1, 3, 7])
def test_live_detector_host_equals_one_detector_per_lane(setting, h):
    probs, times = scripted_probs(), times_ms()
    avg, sup, minc = setting
    host = detector.LiveDetectorHost(3, THRESHOLDS, avg, sup, minc)
    got = [[[] for _ in THRESHOLDS] for _ in range(3)]
    scores = []
    for first, count in push_plan(240, h, leading_empty=2):
        counts, events, sc = host.step(probs[:, first:first + count], times[first:first + count])
        scores.append(sc)
        for k in range(3):
            for j in range(len(THRESHOLDS)):
                assert counts[k, j] == len(events[k][j])
                got[k][j] += [(first + w, f, s) for w, f, s in events[k][j].tolist()]
    for k in range(3):
        for j, thr in enumerate(THRESHOLDS):
            want = lane_reference(probs[k], times, thr, avg, sup, minc)
            assert got[k][j] == want, (k, thr)
            assert sum(f for _, f, _ in want) >= 3, "the scripted stream must fire in every lane"
    assert np.concatenate(scores, axis=1).shape == (3, 240)
    # fired_only keeps the fires
    only = detector.LiveDetectorHost(1, THRESHOLDS[:1], avg, sup, minc, fired_only=True)
    fires = []
    for first, count in push_plan(240, h):
        fires += [(first + w, f, s) for w, f, s in only.step(probs[:1, first:first + count], times[first:first + count])[1][0][0].tolist()]
    assert fires == [e for e in lane_reference(probs[0], times, THRESHOLDS[0], avg, sup, minc) if e[1]]


def test_feed_cuts_any_chunking_into_the_same_pushes():
    audio = np.random.default_rng(1).standard_normal(25600 + 123).astype(np.float32)
    for push in (320, 1280):
        whole = bsa.LivePushCutter(push)
        want = np.concatenate([whole.cut(audio[s:s + 320]) for s in range(0, audio.size, 320)])
        assert want.shape == (audio.size // push, push) and np.array_equal(want.reshape(-1), audio[:want.size])
        ragged, got, at, sizes = bsa.LivePushCutter(push), [], 0, [100, 777, 5000, 1]
        k = 0
        while at < audio.size:
            got.append(ragged.cut(audio[at:at + sizes[k % 4]]))
            at += sizes[k % 4]
            k += 1
        assert np.array_equal(np.concatenate(got), want)
        assert np.array_equal(ragged.rest, audio[want.size:]) and np.array_equal(whole.rest, ragged.rest)
        ragged.reset()
        assert ragged.rest.size == 0 and ragged.cut(audio[:push - 1]).shape == (0, push)


def _longest_deque(avg, hop_samples, rate, n=2000):
    times, best, lo = [(w * hop_samples * 1000) // rate for w in range(n)], 0, 0
    for w, t in enumerate(times):
        while t - avg > times[lo]:
            lo += 1
        best = max(best, w - lo + 1)
    return best


def test_history_rule_and_cap():
    assert [detector.live_history(a, 320, 16000) for a in (100, 40, 0, 300)] == [6, 3, 1, 16]
    for avg, hop, rate in [(100, 320, 16000), (40, 320, 16000), (0, 320, 16000), (300, 320, 16000), (100, 441, 22050), (100, 400, 16000),
                           (37.5, 17, 16000), (250, 147, 44100)]:
        assert 1 <= _longest_deque(avg, hop, rate) <= detector.live_history(avg, hop, rate) <= _longest_deque(avg, hop, rate) + 1
    assert detector.live_history(5118, 320, 16000) == detector.LIVE_MAX_HISTORY == 256
    for bad in (5119, 60000, float("inf")):
        with pytest.raises(ValueError):
            detector.live_history(bad, 320, 16000)
    with pytest.raises(ValueError):
        detector.live_history(-1, 320, 16000)
    with pytest.raises(ValueError):
        detector.live_history(100, 8, 16000)                   # half a millisecond per hop: times repeat
    L = _lib.lib()
    assert L.mkws_detect_live_state_bytes(3, 4, 256) == 3 * (16 + 256 * 16 + 4 * 16) and L.mkws_detect_live_state_bytes(3, 4, 257) == 0
    assert L.mkws_detect_live_state_bytes(3, 0, 6) == 0 and L.mkws_detect_live_state_bytes(3, 1025, 6) == 0
    # the step refuses the cap before it looks at a buffer (the pointers are never followed)
    fake = 64
    step = lambda **kw: L.mkws_detect_live_step(fake, fake, fake, kw.get("max_new", 1), 1, 3, 2, fake, kw.get("n_thr", 1), 100.0, 500.0, 4, 1,
                                                kw.get("history", 6), fake, fake, None, None)
    assert step(history=257) == -2 and b"history" in L.mkws_last_error()
    assert step(history=0) == -1 and step(n_thr=0) == -1 and step(n_thr=1025) == -2 and step(max_new=1025) == -2
