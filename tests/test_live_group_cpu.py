"""The host side of the live group (LiveSessionGroup, mkws_frontend_live_push_many_f32, mkws_detect_live_step_many): the scheduler that
turns chunks for some slots into ticks, the packed many-stream output buffer, and what the wrappers refuse before any device call.  No GPU."""
import numpy as np
import pytest

from multilingual_kws_amd import _lib, detector, frontend
from multilingual_kws_amd.embedding import batch_streaming_analysis as bsa

S = 3


def _feeds(rng, sizes, lengths):
    """Per slot: its audio and the list of chunk lengths it is fed with, one per feed (0 = not fed in that feed)."""
    audio = [rng.standard_normal(n).astype(np.float32) for n in lengths]
    plans = []
    for s in range(S):
        plan, at, k = [], 0, 0
        while at < lengths[s]:
            n = sizes[s][k % len(sizes[s])]
            plan.append(min(n, lengths[s] - at))
            at += plan[-1]
            k += 1
        plans.append(plan)
    return audio, plans


@pytest.mark.parametrize("push", [320, 1280])
@pytest.mark.parametrize("as_dict", [True, False])
def test_scheduler_against_independent_cutters(push, as_dict):
    """Three slots fed ragged chunks of their own sizes; slot 1 gets nothing for the first five feeds.  Tick t of a feed carries the t-th
    push each slot completed in that feed, and every slot's pushes are those of a LivePushCutter of its own fed the same samples whole."""
    rng = np.random.default_rng(3)
    audio, plans = _feeds(rng, [(100, 777, 5000, 1), (1500, 64), (320, 2600, 7)], (25600 + 123, 9000, 25600))
    plans[1] = [0] * 5 + plans[1]
    sched = bsa.LiveGroupScheduler(S, push)
    alone = [bsa.LivePushCutter(push) for _ in range(S)]
    at, got, n_ticks = [0] * S, [[] for _ in range(S)], 0
    for i in range(max(len(p) for p in plans)):
        chunks = {}
        for s in range(S):
            n = plans[s][i] if i < len(plans[s]) else 0
            if n:
                chunks[s] = audio[s][at[s]:at[s] + n]
                at[s] += n
        want = {s: alone[s].cut(c) for s, c in chunks.items()}
        ticks = sched.feed(chunks if as_dict else [chunks.get(s) for s in range(S)])
        assert len(ticks) == max([len(w) for w in want.values()], default=0)        # ticks while any slot has a whole push, and no more
        for t, (active, pushes) in enumerate(ticks):
            assert active.dtype == np.int32 and active.shape == (S,) and pushes.dtype == np.float32 and pushes.shape == (S, push)
            assert active.tolist() == [int(s in want and t < len(want[s])) for s in range(S)] and active.any()
            for s in range(S):
                if active[s]:
                    assert np.array_equal(pushes[s], want[s][t])
                    got[s].append(pushes[s])
        n_ticks += len(ticks)
        assert [sched.pending(s) for s in range(S)] == [alone[s].rest.size for s in range(S)]
    assert n_ticks > 0 and at == [a.size for a in audio]
    for s in range(S):                                                               # the samples fed so far, nothing else, decide the pushes
        whole = bsa.LivePushCutter(push).cut(audio[s])
        assert np.array_equal(np.stack(got[s]), whole) and len(whole) == audio[s].size // push
    sched.reset(2)
    assert sched.pending(2) == 0 and sched.pending(0) == alone[0].rest.size
    sched.reset()
    assert [sched.pending(s) for s in range(S)] == [0] * S and sched.feed({}) == [] and sched.feed([None] * S) == []
    for bad in ({3: audio[0]}, {-1: audio[0]}, [None] * (S + 1)):
        with pytest.raises(ValueError):
            sched.feed(bad)
    with pytest.raises(ValueError):
        bsa.LiveGroupScheduler(0, push)


def test_scheduler_is_independent_of_the_order_and_cut_of_other_slots():
    """The same samples per slot, fed in another interleaving and other chunk sizes: every slot makes the same pushes."""
    rng = np.random.default_rng(4)
    audio = [rng.standard_normal(n).astype(np.float32) for n in (5000, 3333, 4097)]

    def run(order, size):
        sched, got, at = bsa.LiveGroupScheduler(S, 320), [[] for _ in range(S)], [0] * S
        while any(at[s] < audio[s].size for s in range(S)):
            for s in order:
                if at[s] < audio[s].size:
                    for active, pushes in sched.feed({s: audio[s][at[s]:at[s] + size[s]]}):
                        assert active.tolist() == [int(k == s) for k in range(S)]
                        got[s].append(pushes[s].copy())
                    at[s] += size[s]
        return [np.stack(g) for g in got]
    a, b = run((0, 1, 2), (100, 777, 5000)), run((2, 2, 0, 1), (641, 1, 319))
    assert all(np.array_equal(x, y) for x, y in zip(a, b)) and [len(x) for x in a] == [15, 10, 12]


@pytest.mark.parametrize("N,T,h", [(3, 4, 7), (1, 1, 1), (5, 3, 2)])
def test_many_stream_output_buffer_round_trip(N, T, h):
    """The packed buffer (all counts, then all events) against live_unpack per stream."""
    rng = np.random.default_rng(N + T + h)
    counts = rng.integers(0, h + 1, size=(S, N, T)).astype(np.int32)
    events = np.zeros((S, N, T, h), detector.EVENT_DTYPE)
    events["window"], events["fired"], events["score"] = rng.integers(0, h, events.shape), rng.integers(0, 2, events.shape), rng.random(events.shape)
    words = np.zeros(detector.live_out_words_many(S, N, T, h), np.int64)
    cwords = (S * N * T + 1) // 2
    words[:cwords].view(np.int32)[:S * N * T] = counts.reshape(-1)
    words[cwords:] = events.reshape(-1).view(np.int64)
    assert words.size == cwords + 2 * S * N * T * h
    got_counts, got_events = detector.live_unpack_many(words, S, N, T, h)
    assert got_counts.shape == (S, N, T) and got_events.shape == (S, N, T, h)
    for s in range(S):
        one = np.zeros(detector.live_out_words(N, T, h), np.int64)                  # stream s's buffer as detect_live_step would pack it
        one[:(N * T + 1) // 2].view(np.int32)[:N * T] = counts[s].reshape(-1)
        one[(N * T + 1) // 2:] = events[s].reshape(-1).view(np.int64)
        c, e = detector.live_unpack(one, N, T, h)
        assert np.array_equal(got_counts[s], c) and got_events[s].tobytes() == e.tobytes()
    assert detector.live_out_words_many(1, N, T, h) == detector.live_out_words(N, T, h)


def test_wrappers_refuse_bad_strides_and_shapes_before_any_device_call():
    import torch
    N, T, h, history = 3, 4, 2, 6
    need = _lib.lib().mkws_detect_live_state_bytes(N, T, history)
    words = need // 8
    states = torch.zeros((S, words), dtype=torch.int64)
    frontend.check_live_many(states, (S, 2 + h), 2 + h, "meta")
    frontend.check_live_many(torch.zeros((S, words + 3), dtype=torch.int64)[:, :words], (S, 640), 640, "audio")   # a wider row stride is a stride
    for bad_states in (torch.zeros(S * words, dtype=torch.int64), torch.zeros((S, words), dtype=torch.int32),
                       torch.zeros((S, 2 * words), dtype=torch.int64)[:, ::2], torch.zeros((1, words), dtype=torch.int64).expand(S, words)):
        with pytest.raises(ValueError, match="states"):
            frontend.check_live_many(bad_states, (S, 2 + h), 2 + h, "meta")
    with pytest.raises(ValueError, match="audio"):
        frontend.check_live_many(states, (S - 1, 640), 640, "audio")
    with pytest.raises(ValueError, match="audio"):
        frontend.check_live_many(states, None, 640, "audio")
    # detect_live_step_many: every shape rule comes before the first device call (these are host tensors)
    probs, meta, thr = torch.zeros((N, S * h, 3)), torch.zeros((S, 2 + h), dtype=torch.int64), torch.zeros(T, dtype=torch.float64)
    for kw in (dict(meta=meta[0]), dict(meta=meta[:2]), dict(probs=probs[:, :h]), dict(states=states.reshape(-1)), dict(probs=probs)):
        args = dict(states=states, probs=probs, meta=meta)
        args.update(kw)
        with pytest.raises(ValueError):
            detector.detect_live_step_many(args["states"], args["probs"], args["meta"], thr, 100, 500, 4, history)
    # the C call: stride rules and n_streams, refused before a buffer is looked at (the pointers are never followed)
    L, fake = _lib.lib(), 64
    step = lambda stride=need, n=S, **kw: L.mkws_detect_live_step_many(fake, stride, n, fake, fake, kw.get("max_new", h), N, 3, 2, fake, kw.get("n_thr", T),
                                                                        100.0, 500.0, 4, 1, kw.get("history", history), fake, fake, None, None)
    for bad in (0, need - 8, need + 4, 8):
        assert step(stride=bad) == -1 and b"stride" in L.mkws_last_error(), bad
    assert step(n=-1) == -1 and step(n=0) == 0 and step(stride=need + 64, n=0) == 0
    assert step(history=257) == -2 and step(history=0) == -1 and step(n_thr=1025) == -2 and step(max_new=1025) == -2 and step(max_new=0) == 0
    with pytest.raises(ValueError):
        detector.live_detector_state_many(-1, N, T, history)
