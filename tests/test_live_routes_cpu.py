"""The host side of the routed live group (LiveRoutedGroup, mkws_head_group_forward_routes, mkws_detect_live_step_routes): the route table
and its dirty flag, the packed output buffer of R routes, and what the two wrappers refuse before any device call.  No GPU."""
import numpy as np
import pytest

from multilingual_kws_amd import _lib, detector, head
from multilingual_kws_amd.embedding import batch_streaming_analysis as bsa


def test_route_table_fills_the_lowest_free_route_and_tracks_dirt():
    table = bsa.LiveRouteTable(streams=3, n_heads=4, max_routes=4, n_thresholds=2)
    assert table.dirty and table.route_slot.tolist() == [-1] * 4                      # nothing uploaded yet: the first tick uploads
    table.dirty = False
    assert table.attach(2, 1, "hey lamp", (0.5, 0.7)) == 0 and table.dirty
    table.dirty = False
    assert table.attach(0, 3, "ouvre", [0.9, 0.3]) == 1 and table.attach(0, 3, "ouvre", [0.2, 0.1]) == 2 and table.dirty
    assert table.route_slot.tolist() == [2, 0, 0, -1] and table.route_head.tolist()[:3] == [1, 3, 3]
    assert table.thresholds.tolist() == [[0.5, 0.7], [0.9, 0.3], [0.2, 0.1], [0.0, 0.0]] and table.keywords == ["hey lamp", "ouvre", "ouvre", None]
    assert table.routes_of(0) == [1, 2] and table.routes_of(1) == [] and table.routes_of(2) == [0]
    # detach, then attach reuses it (the lowest free one, not the next one)
    table.dirty = False
    table.detach(1)
    assert table.dirty and table.route_slot.tolist() == [2, -1, 0, -1]
    table.dirty = False
    table.detach(1)                                                                   # already free: nothing to upload
    assert not table.dirty
    assert table.attach(1, 0, "uno", (0.4, 0.6)) == 1 and table.dirty
    assert table.attach(1, 2, "dos", (0.4, 0.6)) == 3
    # a refused call changes nothing, the dirty flag included
    table.dirty = False
    with pytest.raises(ValueError, match="full"):
        table.attach(0, 0, "tres", (0.5, 0.5))
    assert not table.dirty
    table.detach(3)
    table.dirty = False
    before = (table.route_slot.copy(), table.route_head.copy(), table.thresholds.copy(), list(table.keywords))
    for bad in (dict(slot=3), dict(slot=-1), dict(head_index=4), dict(head_index=-1), dict(thresholds=(0.5,)), dict(thresholds=(0.5, 0.6, 0.7)),
                dict(thresholds=())):
        args = dict(slot=0, head_index=0, keyword="tres", thresholds=(0.5, 0.5))
        args.update(bad)
        with pytest.raises(ValueError):
            table.attach(**args)
    for bad in (4, -1):
        with pytest.raises(ValueError):
            table.detach(bad)
    assert not table.dirty and table.keywords == before[3]
    assert all(np.array_equal(a, b) for a, b in zip((table.route_slot, table.route_head, table.thresholds), before[:3]))
    for bad in (dict(streams=0), dict(n_heads=0), dict(max_routes=0), dict(n_thresholds=0), dict(n_thresholds=1025)):
        args = dict(streams=3, n_heads=4, max_routes=4, n_thresholds=2)
        args.update(bad)
        with pytest.raises(ValueError):
            bsa.LiveRouteTable(**args)


@pytest.mark.parametrize("R,T", [(4, 2), (5, 1), (3, 3)])
def test_route_table_words_are_one_upload_of_the_three_tables(R, T):
    """route_slot | route_head | thresholds at offsets that are multiples of 8, an odd int32 table padded with one zero."""
    table = bsa.LiveRouteTable(streams=3, n_heads=4, max_routes=R, n_thresholds=T)
    for r in range(R - 1):
        table.attach(r % 3, (r + 1) % 4, f"kw{r}", [0.1 * (r + 1) + 0.01 * k for k in range(T)])
    words, offsets = table.words()
    raw = words.tobytes()
    assert words.dtype == np.int64 and offsets == [0, 8 * ((R + 1) // 2), 16 * ((R + 1) // 2)] and len(raw) == offsets[2] + 8 * R * T
    assert np.array_equal(np.frombuffer(raw, np.int32, R, offsets[0]), table.route_slot) and table.route_slot[-1] == -1
    assert np.array_equal(np.frombuffer(raw, np.int32, R, offsets[1]), table.route_head)
    assert np.array_equal(np.frombuffer(raw, np.float64, R * T, offsets[2]).reshape(R, T), table.thresholds)


@pytest.mark.parametrize("R,T,h", [(7, 4, 3), (1, 1, 1), (5, 3, 2)])
def test_the_packed_buffer_of_routes_is_the_many_stream_layout_with_one_head(R, T, h):
    rng = np.random.default_rng(R + T + h)
    counts = rng.integers(0, h + 1, size=(R, T)).astype(np.int32)
    events = np.zeros((R, T, h), detector.EVENT_DTYPE)
    events["window"], events["fired"], events["score"] = rng.integers(0, h, events.shape), rng.integers(0, 2, events.shape), rng.random(events.shape)
    assert detector.live_out_words_routes(R, T, h) == detector.live_out_words_many(R, 1, T, h) == (R * T + 1) // 2 + 2 * R * T * h
    words = np.zeros(detector.live_out_words_routes(R, T, h), np.int64)
    cwords = (R * T + 1) // 2
    words[:cwords].view(np.int32)[:R * T] = counts.reshape(-1)                        # as mkws_detect_live_step_routes lays them out
    words[cwords:] = events.reshape(-1).view(np.int64)
    got_counts, got_events = detector.live_unpack_many(words, R, 1, T, h)
    assert got_counts.shape == (R, 1, T) and got_events.shape == (R, 1, T, h)
    assert np.array_equal(got_counts[:, 0], counts) and got_events[:, 0].tobytes() == events.tobytes()
    mine = detector.live_unpack_routes(words, R, T, h)
    assert np.array_equal(mine[0], counts) and mine[1].tobytes() == events.tobytes()
    for r in range(R):                                                                # route r alone = a one-stream, one-head buffer
        one = np.zeros(detector.live_out_words(1, T, h), np.int64)
        one[:(T + 1) // 2].view(np.int32)[:T] = counts[r]
        one[(T + 1) // 2:] = events[r].reshape(-1).view(np.int64)
        c, e = detector.live_unpack(one, 1, T, h)
        assert np.array_equal(got_counts[r], c) and got_events[r].tobytes() == e.tobytes()


def test_detect_live_step_routes_refuses_bad_strides_shapes_and_dtypes_before_any_device_call():
    """Host tensors all the way: a device call would fail on them, so every refusal below was decided before one."""
    import torch
    R, S, T, h, history = 5, 3, 4, 2, 6
    need = _lib.lib().mkws_detect_live_state_bytes(1, T, history)
    words = need // 8
    good = dict(states=torch.zeros((R, words), dtype=torch.int64), probs=torch.zeros((R * h, 3)), meta=torch.zeros((S, 2 + h), dtype=torch.int64),
                route_slot=torch.zeros(R, dtype=torch.int32), thresholds=torch.zeros((R, T), dtype=torch.float64))
    assert detector.check_live_routes(**good) == (R, S, h, 3, T)
    assert detector.check_live_routes(**dict(good, probs=torch.zeros((R, h, 3)))) == (R, S, h, 3, T)
    assert detector.check_live_routes(**dict(good, states=torch.zeros((R, words + 3), dtype=torch.int64)[:, :words]))[0] == R    # a wider row stride
    out, scores = torch.zeros(detector.live_out_words_routes(R, T, h), dtype=torch.int64), torch.zeros((R, h), dtype=torch.float64)
    assert detector.check_live_routes(out=out, scores=scores, **good)[0] == R
    bads = [dict(states=torch.zeros(R * words, dtype=torch.int64)), dict(states=torch.zeros((R, words), dtype=torch.int32)),
            dict(states=torch.zeros((R, 2 * words), dtype=torch.int64)[:, ::2]), dict(states=torch.zeros((1, words), dtype=torch.int64).expand(R, words)),
            dict(states=torch.zeros((R - 1, words), dtype=torch.int64)),
            dict(probs=torch.zeros((R * h - 1, 3))), dict(probs=torch.zeros((R * h, 3), dtype=torch.float64)), dict(probs=torch.zeros((R * h, 6))[:, ::2]),
            dict(probs=torch.zeros((R - 1, h, 3))), dict(probs=torch.zeros(R * h * 3)),
            dict(meta=torch.zeros(2 + h, dtype=torch.int64)), dict(meta=torch.zeros((S, 2 + h), dtype=torch.int32)), dict(meta=torch.zeros((S, 1), dtype=torch.int64)),
            dict(meta=torch.zeros((S, 4 + 2 * h), dtype=torch.int64)[:, ::2]),
            dict(route_slot=torch.zeros(R, dtype=torch.int64)), dict(route_slot=torch.zeros(R + 1, dtype=torch.int32)), dict(route_slot=torch.zeros((R, 1), dtype=torch.int32)),
            dict(route_slot=torch.zeros(2 * R, dtype=torch.int32)[::2]),
            dict(thresholds=torch.zeros(T, dtype=torch.float64)), dict(thresholds=torch.zeros((R, T), dtype=torch.float32)),
            dict(thresholds=torch.zeros((R - 1, T), dtype=torch.float64)), dict(thresholds=torch.zeros((R, 0), dtype=torch.float64)),
            dict(thresholds=torch.zeros((R, 2 * T), dtype=torch.float64)[:, ::2]),
            dict(out=out[:-1]), dict(out=out.to(torch.int32)), dict(scores=scores[:, :1]), dict(scores=scores.to(torch.float32))]
    for bad in bads:
        args = dict(good)
        args.update(bad)
        with pytest.raises(ValueError):
            detector.check_live_routes(**args)
        with pytest.raises(ValueError):
            detector.detect_live_step_routes(args["states"], args["probs"], args["meta"], args["route_slot"], args["thresholds"], 100, 500, 4, history,
                                             out=args.get("out"), scores=args.get("scores"))
    with pytest.raises(ValueError, match="CUDA"):                                     # well-shaped host tensors: still no device call
        detector.detect_live_step_routes(good["states"], good["probs"], good["meta"], good["route_slot"], good["thresholds"], 100, 500, 4, history)
    with pytest.raises(ValueError):
        detector.live_detector_state_routes(-1, T, history)
    # the C call: stride rules and sizes, refused before a buffer is looked at (the pointers are never followed)
    L, fake = _lib.lib(), 64
    step = lambda stride=need, n=R, **kw: L.mkws_detect_live_step_routes(fake, stride, n, kw.get("route_slot", fake), kw.get("n_slots", S), fake, fake,
                                                                          kw.get("max_new", h), 3, kw.get("target", 2), fake, kw.get("n_thr", T), 100.0, 500.0, 4, 1,
                                                                          kw.get("history", history), fake, fake, None, None)
    for bad in (0, need - 8, need + 4, 8):
        assert step(stride=bad) == -1 and b"stride" in L.mkws_last_error(), bad
    assert step(n=-1) == -1 and step(n_slots=-1) == -1 and step(route_slot=None) == -1 and step(target=3) == -1 and step(n_thr=0) == -1
    assert step(n=0) == 0 and step(stride=need + 64, n=0) == 0 and step(max_new=0) == 0
    assert step(history=257) == -2 and step(history=0) == -1 and step(n_thr=1025) == -2 and step(max_new=1025) == -2


def test_forward_routes_refuses_bad_shapes_and_dtypes_before_any_device_call():
    import torch
    dev = torch.device("cpu")
    R, S, h = 5, 3, 2
    good = dict(emb=torch.zeros((S * h, 64)), route_slot=torch.zeros(R, dtype=torch.int32), route_head=torch.zeros(R, dtype=torch.int32),
                rows_per_slot=h, n_slots=S)
    assert head.check_forward_routes(64, 3, dev, **good) == (S * h, R)
    assert head.check_forward_routes(64, 3, dev, out=torch.zeros((R, h, 3)), invalid=torch.zeros(1, dtype=torch.int32), **good) == (S * h, R)
    bads = [dict(emb=torch.zeros((S * h, 32))), dict(emb=torch.zeros((S * h, 64), dtype=torch.float64)), dict(emb=torch.zeros((S * h, 128))[:, ::2]),
            dict(emb=torch.zeros(64)), dict(emb=np.zeros((S * h, 64), np.float32)),
            dict(route_slot=torch.zeros(R, dtype=torch.int64)), dict(route_slot=torch.zeros(2 * R, dtype=torch.int32)[::2]), dict(route_slot=[0] * R),
            dict(route_head=torch.zeros(R + 1, dtype=torch.int32)), dict(route_head=torch.zeros((R, 1), dtype=torch.int32)),
            dict(route_head=torch.zeros(R, dtype=torch.float32)),
            dict(rows_per_slot=-1), dict(n_slots=-1),
            dict(out=torch.zeros((R, h, 4))), dict(out=torch.zeros((R * h, 3))), dict(out=torch.zeros((R, h, 3), dtype=torch.float64)),
            dict(out=torch.zeros((R, h, 6))[:, :, ::2]),
            dict(invalid=torch.zeros(2, dtype=torch.int32)), dict(invalid=torch.zeros(1, dtype=torch.int64))]
    for bad in bads:
        args = dict(good)
        args.update(bad)
        with pytest.raises(ValueError, match="forward_routes"):
            head.check_forward_routes(64, 3, dev, **args)
    with pytest.raises(ValueError, match="forward_routes"):                            # another device than the group's
        head.check_forward_routes(64, 3, torch.device("meta"), **good)
    # the C call: a NULL group and (with one) sizes are refused before a buffer is looked at
    L = _lib.lib()
    assert L.mkws_head_group_forward_routes(None, 64, S * h, h, S, 64, 64, R, 64, 64, None) == -1
