"""LiveSessionGroup: S live streams served in lockstep, one device chain per tick.  Each leg is held to code that exists and is tested on
its own: a slot's spectrogram rows to Frontend.stream, a tick's probabilities to the eager embedding + heads on the group's own
spectrograms (same handle), a slot's detections to detect_on_device over the probability rows that slot received, and a group of one
slot to LiveSession row for row."""
import warnings

import numpy as np
import pytest

from multilingual_kws_amd.embedding import batch_streaming_analysis as bsa
from tests.util_data import tone_clip

pytestmark = pytest.mark.gpu
THRESHOLDS = (0.3, 0.5, 0.7)
S, HOP, CLIP, SAMPLES, WINDOWS = 3, 320, 16000, 32000, 51
KEYWORDS = ["uno", "dos", "tres"]


def _recording(seed):
    rng = np.random.default_rng(seed)
    pcm = np.concatenate([tone_clip(400 + 300 * ((k + seed) % 4), rng, n=8000) for k in range(4)])
    return pcm.astype(np.float32) / 32768


@pytest.fixture(scope="module")
def models():
    from multilingual_kws_amd.embedding import transfer_learning as tl
    from multilingual_kws_amd.head import Head
    emb, blob = tl.load_base_model("synthetic", max_batch=16)
    return [tl.TransferLearnedModel(emb, Head(max_batch=16, seed=s), blob, "synthetic") for s in (1, 2, 3)]


@pytest.fixture(scope="module")
def audio():
    return [_recording(9 + s) for s in range(S)]


@pytest.fixture(scope="module")
def stream_spec(audio):
    """Frontend.stream over every slot's whole recording (computed once, shared, not modified)."""
    import torch
    from multilingual_kws_amd.frontend import Frontend
    fe = Frontend(max_samples=SAMPLES)
    want = [fe.stream(torch.from_numpy(a).cuda(), CLIP, HOP) for a in audio]
    torch.cuda.synchronize()
    fe.close()
    return want


def _staggered(audio, push):
    """The feeds of the staggered schedule, one tick each: slot 0 gets a push in every feed, slot 1 none in the first five, slot 2 one in
    every other feed -- each while it has audio left."""
    at, feeds, i = [0] * S, [], 0
    while min(at) < SAMPLES:
        on = [at[0] < SAMPLES, i >= 5 and at[1] < SAMPLES, i % 2 == 0 and at[2] < SAMPLES]
        if any(on):
            feeds.append({s: audio[s][at[s]:at[s] + push] for s in range(S) if on[s]})
        at = [a + push * int(o) for a, o in zip(at, on)]
        i += 1
    return feeds


def _same_cut(audio, sizes):
    """Every slot fed the same chunk lengths: whatever the lengths, tick i is push i of every slot."""
    feeds, at, k = [], 0, 0
    while at < SAMPLES:
        feeds.append([a[at:at + sizes[k % len(sizes)]] for a in audio])
        at += sizes[k % len(sizes)]
        k += 1
    return feeds


def _run(group, feeds, check_probs=False, collect=True):
    """-> per slot (rows, records, the probability rows it received [N, windows, 3], its spectrogram rows); the last two need feeds of one
    tick each (collect=False: None instead)."""
    import torch
    from multilingual_kws_amd.head import Head
    h = group.hops
    rows, records, probs, spec = ([[] for _ in range(S)] for _ in range(4))
    for chunks in feeds:
        before = [group.windows_seen(s) for s in range(S)]
        got = group.feed(chunks)
        fed = sorted(chunks) if isinstance(chunks, dict) else [s for s in range(S) if chunks[s] is not None]
        assert sorted(got) == fed == sorted(group.last_records)
        for s in fed:
            rows[s] += got[s]
            records[s] += group.last_records[s]
        new = [group.windows_seen(s) - before[s] for s in range(S)]
        if check_probs:                                                    # (one tick per feed in the callers that ask for this)
            assert max(new) <= h
            assert torch.equal(group.probs, Head.forward_many(group.heads, group.embedding.forward(group.spec)))
            assert group.meta[:, 0].tolist() == new
        if collect:
            assert max(new) <= h
            for s in range(S):
                probs[s].append(group.probs[:, s * h:s * h + new[s]].clone())
                spec[s].append(group.spec[s * h:s * h + new[s]].clone())
    return [(rows[s], records[s], torch.cat(probs[s], dim=1) if collect else None, torch.cat(spec[s]) if collect else None) for s in range(S)]


def _want_records(group, probs, fired_only):
    from multilingual_kws_amd.detector import detect_on_device
    f, n = group.flags, int(probs.shape[1])
    want = detect_on_device(probs, [20 * w for w in range(n)], THRESHOLDS, f.average_window_duration_ms, f.suppression_ms, f.minimum_count,
                            fired_only=fired_only)
    return sorted((int(w), k, j, int(fired), score) for k in range(3) for j in range(3) for w, fired, score in want.events[k][j].tolist())


@pytest.mark.parametrize("h", [1, 4])
def test_group_equals_its_offline_pieces(models, audio, stream_spec, h):
    import torch
    from multilingual_kws_amd.frontend import live_window_time_ms
    group = bsa.LiveSessionGroup(models, streams=S, thresholds=THRESHOLDS, hops_per_push=h, keywords=KEYWORDS, fired_only=False)
    assert group.graph is not None and [group.samples_seen(s) for s in range(S)] == [0] * S == [group.windows_seen(s) for s in range(S)]
    feeds = _staggered(audio, h * HOP)
    assert sorted(feeds[0]) == [0, 2] and sorted(feeds[1]) == [0] and sorted(feeds[6]) == [0, 1, 2]
    got = _run(group, feeds, check_probs=True)
    assert group.recaptures == 0 and group.fstates[:, 0].tolist() == [SAMPLES] * S
    fired = 0
    for s in range(S):
        rows, records, probs, spec = got[s]
        assert group.windows_seen(s) == WINDOWS == probs.shape[1] and group.samples_seen(s) == SAMPLES and torch.isfinite(probs).all()
        # (a) the slot's spectrogram rows are Frontend.stream's over its audio, (b) its detections detect_on_device's over its probabilities
        assert torch.equal(spec, stream_spec[s])
        want = _want_records(group, probs, False)
        assert records == want, s
        assert rows == [[KEYWORDS[n] if f else "_silence_", live_window_time_ms(w, HOP), score, THRESHOLDS[k]] for w, n, k, f, score in want]
        fired += sum(r[3] for r in records)
    assert fired >= 1, "no keyword fired in any slot: the equalities above would be vacuous"
    # (c) the eager route, same feeds
    eager = bsa.LiveSessionGroup(models, streams=S, thresholds=THRESHOLDS, hops_per_push=h, keywords=KEYWORDS, fired_only=False, use_graph=False)
    assert eager.graph is None
    for mine, theirs in zip(_run(eager, feeds), got):
        assert mine[:2] == theirs[:2] and torch.equal(mine[2], theirs[2]) and torch.equal(mine[3], theirs[3])
    # (d) chunking: every slot fed the same ragged lengths, tick i is push i of every slot whatever the lengths are
    group.reset()
    assert [group.samples_seen(s) for s in range(S)] == [0] * S and not bool(group.fstates.any().cpu()) and not bool(group.dstates.any().cpu())
    whole = [(r, rec) for r, rec, _, _ in _run(group, _same_cut(audio, (h * HOP,)), collect=False)]
    group.reset()
    assert [(r, rec) for r, rec, _, _ in _run(group, _same_cut(audio, (100, 777, 5000, 1)), collect=False)] == whole
    assert sum(len(rec) for _, rec in whole) >= 1
    # fired_only (the default) keeps the fires
    fires = bsa.LiveSessionGroup(models, streams=S, thresholds=THRESHOLDS, hops_per_push=h, keywords=KEYWORDS)
    for (r, rec, _, _), theirs in zip(_run(fires, feeds), got):
        assert r == [x for x, y in zip(theirs[0], theirs[1]) if y[3]] and rec == [y for y in theirs[1] if y[3]]
    for g in (group, eager, fires):
        g.close()


def test_reset_of_a_slot_restarts_only_that_slot(models, audio, stream_spec):
    import torch
    h = 4
    group = bsa.LiveSessionGroup(models, streams=S, thresholds=THRESHOLDS, hops_per_push=h, keywords=KEYWORDS, fired_only=False)
    half = 20 * h * HOP                                                    # 25 600 samples: 31 windows
    first = _run(group, [{s: audio[s][i * h * HOP:(i + 1) * h * HOP] for s in range(S)} for i in range(20)])
    kept = (group.fstates.clone(), group.dstates.clone())
    group.feed({1: audio[1][half:half + 100]})                             # an unfinished push, dropped by the reset
    assert group.samples_seen(1) == half + 100
    group.reset(1)
    assert [group.samples_seen(s) for s in range(S)] == [half, 0, half] and [group.windows_seen(s) for s in range(S)] == [31, 0, 31]
    assert not bool(group.fstates[1].any().cpu()) and not bool(group.dstates[1].any().cpu())
    for s in (0, 2):
        assert torch.equal(group.fstates[s], kept[0][s]) and torch.equal(group.dstates[s], kept[1][s])
    # slot 1 from its start again, the others go on: one push per feed, so that the rows each slot receives can be collected
    feeds = [{0: audio[0][half + i * h * HOP:half + (i + 1) * h * HOP], 1: audio[1][i * h * HOP:(i + 1) * h * HOP],
              2: audio[2][half + i * h * HOP:half + (i + 1) * h * HOP]} for i in range((SAMPLES - half) // (h * HOP))]
    feeds += [{1: audio[1][i * h * HOP:(i + 1) * h * HOP]} for i in range((SAMPLES - half) // (h * HOP), SAMPLES // (h * HOP))]
    second = _run(group, feeds, check_probs=True)
    assert [group.windows_seen(s) for s in range(S)] == [WINDOWS] * S
    # slot 1: a whole stream from window 0 (times and windows restart); slots 0 and 2: the two halves together are one stream
    assert torch.equal(second[1][3], stream_spec[1]) and second[1][1] == _want_records(group, second[1][2], False)
    assert second[1][1] and second[1][1][0][0] < 31
    for s in (0, 2):
        assert torch.equal(torch.cat([first[s][3], second[s][3]]), stream_spec[s])
        assert first[s][1] + second[s][1] == _want_records(group, torch.cat([first[s][2], second[s][2]], dim=1), False)
    with pytest.raises(ValueError):
        group.reset(S)
    group.close()


@pytest.mark.parametrize("h", [1, 4])
def test_a_group_of_one_slot_is_a_live_session(models, audio, h):
    """Same handle, same embedding batch, same plan: the same rows, float64 scores included."""
    group = bsa.LiveSessionGroup(models, streams=1, thresholds=THRESHOLDS, hops_per_push=h, keywords=KEYWORDS, fired_only=False)
    sess = bsa.LiveSession(models, THRESHOLDS, hops_per_push=h, keywords=KEYWORDS, fired_only=False)
    rows, n, at, k, sizes = 0, 0, 0, 0, (h * HOP, 100, 777, 5000, 1)
    while at < SAMPLES:
        chunk = audio[0][at:at + sizes[k % len(sizes)]]
        mine, theirs = group.feed([chunk])[0], sess.feed(chunk)
        assert mine == theirs and group.last_records[0] == sess.last_records, at
        assert group.samples_seen(0) == sess.samples_seen and group.windows_seen(0) == sess.windows_seen
        rows, n, at, k = rows + len(mine), n + sum(r[3] for r in sess.last_records), at + chunk.size, k + 1
    assert group.windows_seen(0) == WINDOWS and rows >= 1 and n >= 1
    group.close()
    sess.close()


def test_constructor_refuses_more_rows_than_the_handle_takes(models):
    for kw in (dict(streams=5, hops_per_push=4), dict(streams=17), dict(streams=0), dict(streams=1, hops_per_push=0)):
        with pytest.raises(ValueError, match="max_batch=16"):
            bsa.LiveSessionGroup(models, thresholds=THRESHOLDS, **kw)
    with pytest.raises(ValueError, match="threshold"):
        bsa.LiveSessionGroup(models, streams=2, thresholds=())
    group = bsa.LiveSessionGroup(models, streams=4, thresholds=THRESHOLDS, hops_per_push=4, use_graph=False)      # 16 rows: the handle's limit
    with pytest.raises(ValueError):
        group.feed({4: np.zeros(10, np.float32)})
    with pytest.raises(ValueError):
        group.feed([None] * 3)
    assert group.feed({}) == {} and group.feed([None] * 4) == {}
    group.close()


def test_group_recaptures_after_a_failed_exchange_without_moving_a_slot(audio, stream_spec):
    """A handle of its own (the healed plan stays with the handle).  The re-capture's warm-up runs the stateful chain: both state tensors
    are put back, so every slot is where its pushes brought it and goes on to detect_on_device's events over the rows it received."""
    import torch
    from multilingual_kws_amd.embedding import transfer_learning as tl
    from multilingual_kws_amd.head import Head
    emb, blob = tl.load_base_model("synthetic", max_batch=16)
    own = [tl.TransferLearnedModel(emb, Head(max_batch=16, seed=s), blob, "synthetic") for s in (1, 2, 3)]
    h = 4
    group = bsa.LiveSessionGroup(own, streams=S, thresholds=THRESHOLDS, hops_per_push=h, keywords=KEYWORDS, fired_only=False)
    feeds = _staggered(audio, h * HOP)
    cut = 16
    first = _run(group, feeds[:cut], check_probs=True)
    where = [group.samples_seen(s) for s in range(S)]
    assert group.recaptures == 0 and where == [cut * h * HOP, (cut - 5) * h * HOP, cut // 2 * h * HOP] and group.windows_seen(0) == 15
    emb.set_option("inject_exchange_error", 1)                              # as if the previous replay's exchange had failed
    assert emb.get_option("exchange_error") != 0
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        second = _run(group, feeds[cut:cut + 1], check_probs=True)
    assert group.recaptures == 1 and emb.get_option("exchange_error") == 0
    moved = [len(feeds[cut].get(s, ())) for s in range(S)]
    assert [group.samples_seen(s) for s in range(S)] == [w + m for w, m in zip(where, moved)] == group.fstates[:, 0].tolist()
    third = _run(group, feeds[cut + 1:], check_probs=True)
    assert group.recaptures == 1 and group.fstates[:, 0].tolist() == [SAMPLES] * S
    n = 0
    for s in range(S):
        spec = torch.cat([first[s][3], second[s][3], third[s][3]])
        probs = torch.cat([first[s][2], second[s][2], third[s][2]], dim=1)
        assert torch.equal(spec, stream_spec[s]) and torch.isfinite(probs).all()
        records = first[s][1] + second[s][1] + third[s][1]
        assert records == _want_records(group, probs, False), s
        n += len(records)
    assert n >= 1
    group.close()
