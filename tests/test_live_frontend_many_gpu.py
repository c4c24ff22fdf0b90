"""mkws_frontend_live_push_many_f32: S live streams advanced by one push each in the same two launches, held to the one-stream forms:
every stream's rows bit for bit to Frontend.stream over its audio, every state slice to a one-stream block fed the same pushes with
live_push, and a stream that is not active in a tick byte for byte to what it was."""
import functools

import numpy as np
import pytest

from multilingual_kws_amd.frontend import Frontend, live_window_time_ms, live_windows
from tests.util_signals import d3_inputs

pytestmark = pytest.mark.gpu
S, CLIP, HOP, SAMPLES = 3, 16000, 320, 25600
ALT = dict(window_size_ms=25, window_step_ms=10, num_channels=32)       # two frames per hop; the carried tail spans more than two steps
CASES = [({}, 1), ({}, 4), (ALT, 4)]


@functools.lru_cache(maxsize=None)
def _signals():
    return d3_inputs()


def _audio(seed):
    """25 600 samples: four 6 400-sample cuts of the shared test signals, which ones, where and how loud decided by the seed."""
    rng, d = np.random.default_rng(seed), _signals()
    parts = []
    for name in rng.permutation(["lcg", "sine1k", "square4", "lcg"]):
        off = int(rng.integers(0, 16000 - 6400))
        parts.append(d[name][off:off + 6400].astype(np.float32) * np.float32(rng.uniform(0.2, 1.0)) / 32768)
    return np.concatenate(parts)


def _schedule(h):
    """active [ticks, S]: stream 0 every tick, stream 1 not in the first five, stream 2 every other tick -- each while it has audio left
    (so every stream also sits through ticks AFTER it has filled its ring).  Ticks: until all three have pushed their 25 600 samples."""
    pushes, done, rows, t = SAMPLES // (h * HOP), [0] * S, [], 0
    while min(done) < pushes:
        on = [done[0] < pushes, t >= 5 and done[1] < pushes, t % 2 == 0 and done[2] < pushes]
        rows.append([int(x) for x in on])
        done = [d + o for d, o in zip(done, rows[-1])]
        t += 1
    return np.asarray(rows, np.int32)


@pytest.mark.parametrize("over,h", CASES)
def test_many_streams_equal_the_one_stream_forms(over, h):
    import torch
    fe = Frontend(max_samples=SAMPLES, **over)
    audio = [_audio(11 + s) for s in range(S)]
    assert not np.array_equal(audio[0], audio[1])
    d_audio = [torch.from_numpy(a).cuda() for a in audio]
    want = [tuple(x.cpu().numpy() for x in fe.stream(a, CLIP, HOP, want_raw=True)) for a in d_audio]
    W = live_windows(SAMPLES, CLIP, HOP)
    assert W == 31 == want[0][0].shape[0]
    F, C, P = want[0][0].shape[1], fe.num_channels, h * HOP
    sched = _schedule(h)
    ticks = sched.shape[0]
    assert sched[:5, 1].sum() == 0 and sched[:, 2].tolist()[:4] == [1, 0, 1, 0] and sched.sum(0).tolist() == [SAMPLES // P] * S
    # states with a row stride WIDER than a state block: the five words behind every slice are not the call's to touch
    words = fe.live_state(CLIP, HOP, h).numel()
    block = torch.full((S, words + 5), 0x5A5A5A5A, dtype=torch.int64, device="cuda")
    states = block[:, :words]
    states.zero_()
    assert fe.live_state_many(S, CLIP, HOP, h).shape == (S, words)
    spec = torch.full((ticks, S * h, F, C), -1.0, dtype=torch.float32, device="cuda")
    raw = torch.full((ticks, S * h, F, C), -1, dtype=torch.int16, device="cuda")
    meta = torch.full((ticks, S, 2 + h), -1, dtype=torch.int64, device="cuda")
    d_sched = torch.from_numpy(sched).cuda()
    pushed = [0] * S
    junk = torch.full((P,), float("nan"), dtype=torch.float32, device="cuda")      # the audio row of a stream that is not active: not read
    kept = torch.ones((), dtype=torch.bool, device="cuda")
    for t in range(ticks):                                                         # no synchronisation in between
        rows = torch.stack([d_audio[s][pushed[s] * P:(pushed[s] + 1) * P] if sched[t, s] else junk for s in range(S)])
        before = states.clone()
        fe.live_push_many(states, rows, CLIP, HOP, h, active=d_sched[t], spec=spec[t], raw=raw[t], meta=meta[t])
        for s in range(S):
            if not sched[t, s]:
                kept &= (states[s] == before[s]).all()                             # (compared on the device: no synchronisation)
            pushed[s] += int(sched[t, s])
    assert bool(kept.cpu()), "the state slice of a stream that was not active changed"
    assert bool((block[:, words:] == 0x5A5A5A5A).all().cpu()), "the call wrote between two state slices"
    spec, raw, meta = spec.cpu().numpy(), raw.cpu().numpy(), meta.cpu().numpy()
    ragged = 0
    for s in range(S):
        seen, emitted = 0, 0
        for t in range(ticks):
            mine = slice(s * h, (s + 1) * h)
            first = live_windows(seen, CLIP, HOP)
            if not sched[t, s]:
                # not advanced: count = 0 with the window the stream is at, every row of its spec / raw as it was
                assert meta[t, s].tolist() == [0, first] + [-1] * h, (s, t)
                assert (spec[t, mine] == -1).all() and (raw[t, mine] == -1).all(), (s, t)
                continue
            after = live_windows(seen + P, CLIP, HOP)
            count = after - first
            ragged += 0 < count < h
            assert meta[t, s].tolist() == [count, first] + [live_window_time_ms(w, HOP) for w in range(first, after)] + [-1] * (h - count), (s, t)
            assert np.array_equal(spec[t, mine][:count], want[s][0][first:after]) and np.array_equal(raw[t, mine][:count], want[s][1][first:after]), (s, t)
            assert (spec[t, mine][count:] == -1).all() and (raw[t, mine][count:] == -1).all(), (s, t)    # rows past count are left untouched
            seen, emitted = seen + P, emitted + count
        assert seen == SAMPLES and emitted == W
    assert ragged == (S if h == 4 else 0)                                  # 13 pushes of 1 280 samples complete three windows
    # every slice is the block a one-stream call leaves after the same pushes
    for s in range(S):
        one = fe.live_state(CLIP, HOP, h)
        for i in range(SAMPLES // P):
            fe.live_push(one, d_audio[s][i * P:(i + 1) * P], CLIP, HOP, h)
        assert torch.equal(states[s], one), s
        assert int(states[s, 0].cpu()) == SAMPLES
    fe.close()


def test_a_slice_moves_between_the_two_calls_and_all_active_is_the_default():
    """active = None advances every stream; a slice copied out, pushed with the one-stream call and copied back continues in the group."""
    import torch
    h, P = 1, HOP
    fe = Frontend(max_samples=SAMPLES)
    d_audio = torch.stack([torch.from_numpy(_audio(21 + s)) for s in range(S)]).cuda()
    want = [fe.stream(d_audio[s], CLIP, HOP) for s in range(S)]
    states = fe.live_state_many(S, CLIP, HOP, h)
    rows = [[] for _ in range(S)]
    for i in range(SAMPLES // P):
        if i == 55:                                                        # stream 1 takes this push on its own
            one = states[1].clone()
            sp, _, me = fe.live_push(one, d_audio[1, i * P:(i + 1) * P], CLIP, HOP, h)
            states[1].copy_(one)
            rows[1].append(sp[:int(me[0].cpu())].clone())
            active = torch.tensor([1, 0, 1], dtype=torch.int32, device="cuda")
        else:
            active = None
        sp, none, me = fe.live_push_many(states, d_audio[:, i * P:(i + 1) * P].contiguous(), CLIP, HOP, h, active=active)
        assert none is None
        me = me.cpu()
        for s in range(S):
            rows[s].append(sp[s * h:s * h + int(me[s, 0])].clone())
    for s in range(S):
        assert torch.equal(torch.cat(rows[s]), want[s]), s
    fe.close()


def test_live_push_many_refuses_what_it_documents():
    import torch
    fe = Frontend(max_samples=SAMPLES)
    h = 2
    states = fe.live_state_many(S, CLIP, HOP, h)
    need = fe.L.mkws_frontend_live_state_bytes(fe.h, CLIP, HOP, h)
    assert 8 * states.shape[1] == (need + 7) // 8 * 8
    audio = torch.zeros((S, h * HOP), dtype=torch.float32, device="cuda")
    spec, _, meta = fe.live_push_many(states, audio, CLIP, HOP, h)
    assert tuple(spec.shape) == (S * h, 49, 40) and meta[:, :2].tolist() == [[0, 0]] * S and states[:, 0].tolist() == [h * HOP] * S

    def push(ptr=states.data_ptr(), stride=8 * states.shape[1], n=S, hop=HOP, hops=h, spec_ptr=spec.data_ptr(), meta_ptr=meta.data_ptr()):
        return fe.L.mkws_frontend_live_push_many_f32(fe.h, ptr, stride, n, None, audio.data_ptr(), CLIP, hop, hops, spec_ptr, None, meta_ptr, None)
    before = states.clone()
    for bad in (dict(stride=0), dict(stride=need - 8), dict(stride=8 * states.shape[1] + 4), dict(n=-1), dict(ptr=None), dict(hops=0),
                dict(spec_ptr=None), dict(meta_ptr=None)):
        assert push(**bad) == -1, bad
    assert push(hop=300) == -2                                             # not a multiple of the frame step
    assert push(n=0) == 0
    torch.cuda.synchronize()
    assert torch.equal(states, before)                                     # nothing was launched
    with pytest.raises(ValueError, match="audio"):
        fe.live_push_many(states, audio[:2], CLIP, HOP, h)
    with pytest.raises(ValueError, match="audio"):
        fe.live_push_many(states, audio[:, :HOP].contiguous(), CLIP, HOP, h)
    with pytest.raises(ValueError, match="active"):
        fe.live_push_many(states, audio, CLIP, HOP, h, active=torch.ones(S, dtype=torch.int64, device="cuda"))
    with pytest.raises(ValueError, match="states"):
        fe.live_push_many(states.reshape(-1), audio, CLIP, HOP, h)
    with pytest.raises(ValueError, match="meta"):
        fe.live_push_many(states, audio, CLIP, HOP, h, meta=torch.zeros(2 + h, dtype=torch.int64, device="cuda"))
    with pytest.raises(ValueError, match="frame step"):
        fe.live_state_many(S, CLIP, 300, h)
    fe.close()
