"""LiveRoutedGroup: S live streams whose slots each spot their own keywords through a route table in device memory.  With every slot routed
to every head it is held to LiveSessionGroup row for row; with personal routes every route is held to Head.forward of its head on its
slot's embedding rows and to detect_on_device over the rows it received since it was attached; the table is edited in mid-stream without a
re-capture."""
import warnings

import numpy as np
import pytest

from multilingual_kws_amd.embedding import batch_streaming_analysis as bsa
from tests.util_data import tone_clip

pytestmark = pytest.mark.gpu
THRESHOLDS = (0.3, 0.5, 0.7)
S, HOP, CLIP, SAMPLES, WINDOWS = 3, 320, 16000, 32000, 51
KEYWORDS = ["uno", "dos", "tres", "cuatro"]


def _recording(seed):
    rng = np.random.default_rng(seed)
    pcm = np.concatenate([tone_clip(400 + 300 * ((k + seed) % 4), rng, n=8000) for k in range(4)])
    return pcm.astype(np.float32) / 32768


@pytest.fixture(scope="module")
def handle():
    from multilingual_kws_amd.embedding import transfer_learning as tl
    from multilingual_kws_amd.head import Head
    emb, _ = tl.load_base_model("synthetic", max_batch=16)
    return emb, [Head(max_batch=16, seed=s) for s in (1, 2, 3, 4)]


@pytest.fixture(scope="module")
def audio():
    return [_recording(9 + s) for s in range(S)]


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
    feeds, at, k = [], 0, 0
    while at < SAMPLES:
        feeds.append([a[at:at + sizes[k % len(sizes)]] for a in audio])
        at += sizes[k % len(sizes)]
        k += 1
    return feeds


def _run(group, feeds, collect=True, check_probs=False, before=None):
    """-> per slot (rows, records) and, with collect (feeds of one tick each), per (route, slot, head) the probability rows that route
    received while it was attached so, [windows, 3], with the slot's window its first row belongs to.  before(i): called before feed i (the
    mid-stream edits)."""
    import torch
    h = group.hops
    rows, records = [[] for _ in range(S)], [[] for _ in range(S)]
    heard = {}
    for i, chunks in enumerate(feeds):
        if before is not None:
            before(i)
        seen = [group.windows_seen(s) for s in range(S)]
        table, heads_of = group.table.route_slot.copy(), group.table.route_head.copy()     # what this feed's tick will run with
        got = group.feed(chunks)
        fed = sorted(chunks) if isinstance(chunks, dict) else [s for s in range(S) if chunks[s] is not None]
        assert sorted(got) == fed == sorted(group.last_records)
        for s in fed:
            rows[s] += got[s]
            records[s] += group.last_records[s]
        new = [group.windows_seen(s) - seen[s] for s in range(S)]
        if collect or check_probs:
            assert max(new) <= h and group.meta[:, 0].tolist() == new and int(group.invalid.cpu()[0]) == 0
        if check_probs:                                                    # every attached route: its head on its slot's rows, same handle
            emb = group.embedding.forward(group.spec)
            for r in np.flatnonzero(table >= 0).tolist():
                s = int(table[r])
                want = group.heads[int(heads_of[r])].forward(emb[s * h:(s + 1) * h])
                assert torch.equal(group.probs[r], want), (i, r)
        if collect:
            for r in np.flatnonzero(table >= 0).tolist():
                s = int(table[r])
                if new[s]:
                    _, parts = heard.setdefault((r, s, int(heads_of[r])), (seen[s], []))
                    parts.append(group.probs[r, :new[s]].clone())
    return [(rows[s], records[s]) for s in range(S)], {key: (first, torch.cat(parts)) for key, (first, parts) in heard.items()}


def _of_route(records, r):
    return [(w, k, fired, score) for w, route, k, fired, score, _, _ in records if route == r]


def _want(group, first, probs, thresholds, fired_only):
    """detect_on_device over the rows a route received, at its slot's window times -> sorted [(window, threshold index, fired, score)]."""
    from multilingual_kws_amd.detector import detect_on_device
    f, n = group.flags, int(probs.shape[0])
    want = detect_on_device(probs[None], [20 * w for w in range(first, first + n)], list(thresholds), f.average_window_duration_ms, f.suppression_ms,
                            f.minimum_count, fired_only=fired_only)
    return sorted((first + int(w), k, int(fired), score) for k in range(len(thresholds)) for w, fired, score in want.events[0][k].tolist())


def _rows_of(records):
    return [[kw if fired else "_silence_", 20 * w, score, thr] for w, _, _, fired, score, kw, thr in records]


@pytest.mark.parametrize("h", [1, 4])
def test_every_slot_routed_to_every_head_is_the_unrouted_group(handle, audio, h):
    """Same handle, same embedding batch, same head kernel per row, same detector per lane: the same rows, float64 scores bit-equal; only the
    order within a window differs (route id there, head index here)."""
    emb, heads = handle
    routed = bsa.LiveRoutedGroup(emb, heads, S, max_routes=S * len(heads), n_thresholds=len(THRESHOLDS), hops_per_push=h, fired_only=False)
    for s in range(S):
        for n in range(len(heads)):
            assert routed.attach(s, n, KEYWORDS[n], THRESHOLDS) == s * len(heads) + n
    plain = bsa.LiveSessionGroup(streams=S, thresholds=THRESHOLDS, hops_per_push=h, embedding=emb, heads=heads, keywords=KEYWORDS, fired_only=False)
    fires = 0
    for chunks in _staggered(audio, h * HOP):
        mine, theirs = routed.feed(chunks), plain.feed(chunks)
        assert sorted(mine) == sorted(theirs)
        key = lambda row: (row[1], row[3], row[0], row[2])                 # (window time, threshold, keyword, score)
        for s in mine:
            assert sorted(mine[s], key=key) == sorted(theirs[s], key=key), s
            a = sorted((w, int(routed.table.route_head[r]), k, fired, score) for w, r, k, fired, score, _, _ in routed.last_records[s])
            assert a == sorted(plain.last_records[s]), s
            assert [rec[0] for rec in routed.last_records[s]] == sorted(rec[0] for rec in routed.last_records[s])      # ordered by window ...
            assert routed.last_records[s] == sorted(routed.last_records[s], key=lambda rec: rec[:3])                     # ... route id, threshold
            fires += sum(rec[3] for rec in routed.last_records[s])
    assert fires >= 1 and routed.recaptures == 0 and [routed.windows_seen(s) for s in range(S)] == [WINDOWS] * S
    routed.close()
    plain.close()


def _personal(emb, heads, h, **kw):
    group = bsa.LiveRoutedGroup(emb, heads, S, max_routes=5, n_thresholds=2, hops_per_push=h, fired_only=False, **kw)
    assert group.attach(0, 0, "uno", (0.3, 0.5)) == 0 and group.attach(0, 1, "dos", (0.3, 0.5)) == 1 and group.attach(1, 2, "tres", (0.4, 0.6)) == 2
    return group


PERSONAL = {0: (0, (0.3, 0.5)), 1: (0, (0.3, 0.5)), 2: (1, (0.4, 0.6))}       # route: (slot, thresholds)
KEY = {0: (0, 0, 0), 1: (1, 0, 1), 2: (2, 1, 2)}                              # route: its key in what _run collects (route, slot, head)


@pytest.mark.parametrize("h", [1, 4])
def test_personal_routes_equal_their_offline_pieces(handle, audio, h):
    import torch
    emb, heads = handle
    group = _personal(emb, heads, h)
    assert group.graph is not None
    graph = group.graph
    feeds = _staggered(audio, h * HOP)
    got, heard = _run(group, feeds, check_probs=True)
    assert sorted(heard) == sorted(KEY.values()) and group.recaptures == 0 and group.graph is graph
    fired = 0
    for r, (slot, thr) in PERSONAL.items():
        first, probs = heard[KEY[r]]
        assert first == 0 and probs.shape[0] == WINDOWS and torch.isfinite(probs).all()
        mine = _of_route(got[slot][1], r)
        assert mine == _want(group, 0, probs, thr, False), r
        fired += sum(x[2] for x in mine)
    assert fired >= 1, "no keyword fired on any route: the equalities above would be vacuous"
    for s in range(S):
        assert got[s][0] == _rows_of(got[s][1])
        assert got[s][1] == sorted(got[s][1], key=lambda rec: rec[:3])
    assert got[2] == ([], []) and {rec[5] for rec in got[0][1]} <= {"uno", "dos"} and {rec[5] for rec in got[1][1]} <= {"tres"}
    assert {rec[6] for rec in got[1][1]} <= {0.4, 0.6}
    # the eager route, same feeds
    eager = _personal(emb, heads, h, use_graph=False)
    assert eager.graph is None
    e_got, e_heard = _run(eager, feeds)
    assert e_got == got and sorted(e_heard) == sorted(heard) and all(torch.equal(e_heard[key][1], heard[key][1]) for key in heard)
    # chunking: every slot fed the same ragged lengths, tick i is push i of every slot whatever the lengths are
    group.reset()
    assert not bool(group.fstates.any().cpu()) and not bool(group.dstates.any().cpu()) and [group.samples_seen(s) for s in range(S)] == [0] * S
    whole, _ = _run(group, _same_cut(audio, (h * HOP,)), collect=False)
    group.reset()
    ragged, _ = _run(group, _same_cut(audio, (100, 777, 5000, 1)), collect=False)
    assert ragged == whole and sum(len(rec) for _, rec in whole) >= 1 and group.graph is graph
    # fired_only (the default) keeps the fires
    fires = bsa.LiveRoutedGroup(emb, heads, S, max_routes=5, n_thresholds=2, hops_per_push=h)
    for r, (slot, thr) in PERSONAL.items():
        fires.attach(slot, r, ["uno", "dos", "tres"][r], thr)
    f_got, _ = _run(fires, feeds, collect=False)
    for s in range(S):
        assert f_got[s][1] == [rec for rec in got[s][1] if rec[3]] and f_got[s][0] == [row for row, rec in zip(got[s][0], got[s][1]) if rec[3]]
    for g in (group, eager, fires):
        g.close()


def test_attach_detach_and_set_params_in_mid_stream_do_not_recapture(handle, audio):
    """Two runs over the same feeds: one left alone, one whose table is edited before feed EDIT -- route 1 detached, spare head 3 given new
    parameters and attached to slot 2 in the freed route.  The other routes do not notice; the new route is a fresh detector over the rows
    since its attach."""
    import torch
    from multilingual_kws_amd.head import Head, glorot_uniform_params
    emb, heads = handle
    h, EDIT, NEW_THR = 4, 18, (0.2, 0.35)
    feeds = [{s: audio[s][i * h * HOP:(i + 1) * h * HOP] for s in range(S)} for i in range(SAMPLES // (h * HOP))]
    kept = heads[3].get_params()
    alone = _personal(emb, heads, h)
    a_got, _ = _run(alone, feeds)
    edited = _personal(emb, heads, h)
    graph = edited.graph
    new_params = glorot_uniform_params(seed=77)
    at = {}

    def before(i):
        if i == EDIT:
            assert not edited.table.dirty
            at["window"] = edited.windows_seen(2)
            edited.detach(1)
            assert edited.table.dirty
            heads[3].set_params(new_params)
            assert edited.attach(2, 3, "nuevo", NEW_THR) == 1                                   # the lowest free route
    try:
        e_got, e_heard = _run(edited, feeds, check_probs=True, before=before)
        assert edited.graph is graph and edited.recaptures == 0 and not edited.table.dirty and at["window"] == 23
        # the routes that were not edited: the same rows as without the edit
        for s, keyword in ((0, "uno"), (1, "tres")):
            pick = lambda got: [(row, rec) for row, rec in zip(*got) if rec[5] == keyword]
            assert pick(e_got[s]) == pick(a_got[s]) and len(pick(a_got[s])) >= 1 and pick(a_got[s])[-1][1][0] >= at["window"]
        # the detached route: what it reported before the edit, nothing after (the slots are in lockstep: the same window everywhere)
        dos_alone, dos_edited = [rec for rec in a_got[0][1] if rec[5] == "dos"], [rec for rec in e_got[0][1] if rec[5] == "dos"]
        assert dos_edited == [rec for rec in dos_alone if rec[0] < at["window"]] and len(dos_alone) > len(dos_edited) >= 1
        # the new route: from its attach on, head 3's NEW parameters on slot 2's rows, a fresh detector
        assert sorted(e_heard) == [(0, 0, 0), (1, 0, 1), (1, 2, 3), (2, 1, 2)]
        first, probs = e_heard[(1, 2, 3)]
        assert first == at["window"] and probs.shape[0] == WINDOWS - first and a_got[2] == ([], [])
        assert all(rec[5] == "nuevo" and rec[1] == 1 and rec[0] >= first for rec in e_got[2][1])
        assert _of_route(e_got[2][1], 1) == _want(edited, first, probs, NEW_THR, False) and len(e_got[2][1]) >= 1
        fresh = Head(max_batch=16, params=new_params)
        rows = edited.embedding.forward(edited.spec)[2 * h:3 * h]
        assert torch.equal(edited.probs[1], fresh.forward(rows)) and not torch.equal(edited.probs[1], Head(max_batch=16, params=kept).forward(rows))
    finally:
        heads[3].set_params(kept)
    alone.close()
    edited.close()


def test_reset_of_a_slot_restarts_that_slot_and_the_detectors_of_its_routes(handle, audio):
    import torch
    emb, heads = handle
    h = 4
    group = _personal(emb, heads, h)
    half = 20 * h * HOP                                                    # 25 600 samples: 31 windows
    first, heard1 = _run(group, [{s: audio[s][i * h * HOP:(i + 1) * h * HOP] for s in range(S)} for i in range(20)])
    kept = (group.fstates.clone(), group.dstates.clone())
    group.feed({0: audio[0][half:half + 100]})                             # an unfinished push, dropped by the reset
    assert group.samples_seen(0) == half + 100
    group.reset(0)
    assert [group.samples_seen(s) for s in range(S)] == [0, half, half] and [group.windows_seen(s) for s in range(S)] == [0, 31, 31]
    assert not bool(group.fstates[0].any().cpu()) and not bool(group.dstates[0].any().cpu()) and not bool(group.dstates[1].any().cpu())
    assert torch.equal(group.fstates[1:], kept[0][1:]) and torch.equal(group.dstates[2:], kept[1][2:]) and bool(group.dstates[2].any().cpu())
    n = (SAMPLES - half) // (h * HOP)
    feeds = [{0: audio[0][i * h * HOP:(i + 1) * h * HOP], 1: audio[1][half + i * h * HOP:half + (i + 1) * h * HOP]} for i in range(n)]
    feeds += [{0: audio[0][i * h * HOP:(i + 1) * h * HOP]} for i in range(n, SAMPLES // (h * HOP))]
    second, heard2 = _run(group, feeds, check_probs=True)
    assert [group.windows_seen(s) for s in range(S)] == [WINDOWS, WINDOWS, 31]
    # slot 0's routes: whole streams from window 0; slot 1's route: the two halves together are one stream
    for r in (0, 1):
        assert heard2[KEY[r]][0] == 0 and _of_route(second[0][1], r) == _want(group, 0, heard2[KEY[r]][1], PERSONAL[r][1], False)
    both = torch.cat([heard1[KEY[2]][1], heard2[KEY[2]][1]])
    assert heard2[KEY[2]][0] == 31 and _of_route(first[1][1] + second[1][1], 2) == _want(group, 0, both, PERSONAL[2][1], False)
    assert len(second[0][1]) >= 1
    with pytest.raises(ValueError):
        group.reset(S)
    group.close()


def test_the_routed_group_refuses_what_it_documents(handle):
    emb, heads = handle
    for kw in (dict(streams=5, hops_per_push=4), dict(streams=17), dict(streams=0), dict(streams=1, hops_per_push=0)):
        with pytest.raises(ValueError, match="max_batch=16"):
            bsa.LiveRoutedGroup(emb, heads, max_routes=4, **kw)
    for kw in (dict(max_routes=0), dict(n_thresholds=0)):
        with pytest.raises(ValueError):
            bsa.LiveRoutedGroup(emb, heads, S, **dict(dict(max_routes=4), **kw))
    group = bsa.LiveRoutedGroup(emb, heads, S, max_routes=2, use_graph=False)
    assert group.feed({0: np.zeros(HOP, np.float32), 2: np.zeros(10, np.float32)}) == {0: [], 2: []}      # no route yet: nobody listens
    assert group.attach(0, 0, "uno", [0.5]) == 0 and group.attach(2, 3, "dos", 0.6) == 1
    for bad in (dict(slot=S), dict(head_index=len(heads)), dict(thresholds=(0.5, 0.6))):
        with pytest.raises(ValueError):
            group.attach(**dict(dict(slot=0, head_index=0, keyword="x", thresholds=(0.5,)), **bad))
    group.detach(0)
    with pytest.raises(ValueError, match="full"):
        group.attach(0, 0, "a", [0.5]), group.attach(0, 0, "b", [0.5])
    with pytest.raises(ValueError):
        group.detach(2)
    with pytest.raises(ValueError):
        group.feed({S: np.zeros(10, np.float32)})
    assert group.feed({}) == {}
    group.close()


def test_routed_group_recaptures_after_a_failed_exchange_without_moving_a_slot(audio):
    """A handle of its own (the healed plan stays with the handle).  The re-capture's warm-up runs the stateful chain: both state tensors
    are put back, so every slot is where its pushes brought it and every route goes on to detect_on_device's events over the rows it
    received."""
    import torch
    from multilingual_kws_amd.embedding import transfer_learning as tl
    from multilingual_kws_amd.head import Head
    emb, _ = tl.load_base_model("synthetic", max_batch=16)
    heads = [Head(max_batch=16, seed=s) for s in (1, 2, 3, 4)]
    h = 4
    group = _personal(emb, heads, h)
    feeds = _staggered(audio, h * HOP)
    cut = 16
    first, heard1 = _run(group, feeds[:cut], check_probs=True)
    where = [group.samples_seen(s) for s in range(S)]
    assert group.recaptures == 0 and where == [cut * h * HOP, (cut - 5) * h * HOP, cut // 2 * h * HOP] and group.windows_seen(0) == 15
    emb.set_option("inject_exchange_error", 1)                              # as if the previous replay's exchange had failed
    assert emb.get_option("exchange_error") != 0
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        second, heard2 = _run(group, feeds[cut:cut + 1], check_probs=True)
    assert group.recaptures == 1 and emb.get_option("exchange_error") == 0
    moved = [len(feeds[cut].get(s, ())) for s in range(S)]
    assert [group.samples_seen(s) for s in range(S)] == [w + m for w, m in zip(where, moved)] == group.fstates[:, 0].tolist()
    third, heard3 = _run(group, feeds[cut + 1:], check_probs=True)
    assert group.recaptures == 1 and group.fstates[:, 0].tolist() == [SAMPLES] * S
    n = 0
    for r, (slot, thr) in PERSONAL.items():
        probs = torch.cat([x[KEY[r]][1] for x in (heard1, heard2, heard3) if KEY[r] in x])
        assert probs.shape[0] == WINDOWS and torch.isfinite(probs).all()
        records = _of_route(first[slot][1] + second[slot][1] + third[slot][1], r)
        assert records == _want(group, 0, probs, thr, False), r
        n += len(records)
    assert n >= 1
    group.close()
