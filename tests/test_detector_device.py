"""The device detector (mkws_detect_stream / detector.detect_on_device / batch_streaming_analysis.detect_many) against the host class
SingleTargetRecognizeCommands.  Every comparison is exact: labels, event windows, is_new_command, and the scores bit-equal as float64
(NaN matching NaN) -- both sides perform the same IEEE operations in the same order, so there is no tolerance to choose."""
import json
import os

import numpy as np
import pytest

from multilingual_kws_amd.embedding import batch_streaming_analysis as sa
from multilingual_kws_amd.embedding.single_target_recognize_commands import RecognizeResult, SingleTargetRecognizeCommands

LABELS = ["_silence_", "_unknown_", "kw"]


def _host_steps(probs, times, thr, avg, sup, minc):
    """One keyword, one threshold on the host: per window (is keyword, is_new_command, score)."""
    rc = SingleTargetRecognizeCommands(LABELS, avg, thr, sup, minc, 2)
    el = RecognizeResult()
    kw, new, score = [], [], []
    for row, t in zip(probs, times):
        rc.process_latest_result(row, int(t), el)
        kw.append(el.found_command == "kw")
        new.append(bool(el.is_new_command))
        score.append(float(el.score))
    return np.array(kw, bool), np.array(new, bool), np.array(score, np.float64)


def _same(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and bool(np.all((a == b) | (np.isnan(a) & np.isnan(b))))


def _bursty(n, seed, centres, width=8):
    rng = np.random.default_rng(seed)
    tgt = np.full(n, 0.02)
    for c in centres:
        tgt[max(0, c - width):c + width] = 0.97
    other = rng.uniform(0, 1, n) * (1 - tgt)
    return np.stack([1 - tgt - other, other, tgt], axis=1).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------- without a GPU

def test_detect_many_equals_detect_per_keyword_and_threshold():
    n = 240
    flags = sa.StreamFlags(wav="unused.wav", ground_truth="", target_keyword="mask", detection_thresholds=[0.5, 0.9])
    per_kw = {"alpha": _bursty(n, 1, [40, 120]), "beta": _bursty(n, 2, [20, 90, 200]), "gamma": _bursty(n, 3, [])}
    thresholds = [0.3, 0.5, 0.9]
    import dataclasses
    want = [{t: sa.detect(inf, dataclasses.replace(flags, target_keyword=kw), t) for t in thresholds} for kw, inf in per_kw.items()]
    assert sum(len(w[0.9][0]) for w in want) >= 4
    assert sa.detect_many(list(per_kw.values()), flags, thresholds, keywords=list(per_kw)) == want
    assert sa.detect_many(np.stack(list(per_kw.values())), flags, thresholds, keywords=list(per_kw)) == want
    one = sa.detect_many(per_kw["beta"], flags, thresholds)
    assert one == {t: sa.detect(per_kw["beta"], flags, t) for t in thresholds} and list(one) == thresholds
    assert all(type(c) is float for _, _, c in one[0.5][1]) and all(type(t) is int for _, t in one[0.5][0])
    # more rows than window offsets are cut to the offsets; fewer raise as detect() does
    data_samples = 16000 + 320 * 100                                       # 100 windows
    assert len(sa.window_offsets(data_samples, 16000, 320)) == 100
    cut = sa.detect_many(per_kw["alpha"], flags, thresholds, data_samples=data_samples)
    assert cut == {t: sa.detect(per_kw["alpha"], flags, t, data_samples=data_samples) for t in thresholds}
    assert cut == sa.detect_many(per_kw["alpha"][:100], flags, thresholds) and cut != sa.detect_many(per_kw["alpha"], flags, thresholds)
    with pytest.raises(IndexError):
        sa.detect(per_kw["alpha"][:50], flags, 0.5, data_samples=data_samples)
    with pytest.raises(IndexError):
        sa.detect_many(per_kw["alpha"][:50], flags, thresholds, data_samples=data_samples)
    with pytest.raises(ValueError):
        sa.detect_many(list(per_kw.values()), flags, thresholds, keywords=["a", "b"])


def test_detect_on_device_refuses_decreasing_times_before_touching_the_device():
    from multilingual_kws_amd.detector import check_times, detect_on_device, event_capacity
    probs = np.zeros((1, 4, 3), np.float32)
    with pytest.raises(ValueError, match="Results must be fed in increasing time order, but receive a timestamp of 30, which was "
                                         "earlier than the previous one of 40"):
        detect_on_device(probs, [0, 20, 40, 30], [0.5], 100, 500, 4)
    assert check_times([0, 20, 20, 45]).dtype == np.int64
    # the bound of the wrapper's event buffer: two state changes per suppression_ms, one fire per suppression_ms
    t = np.arange(2950) * 20
    assert event_capacity(t, 500) == 2 * (58980 // 500) + 2 and event_capacity(t, 500, fired_only=True) == 58980 // 500 + 2
    assert event_capacity(t, 0) == 2950 and event_capacity(t[:3], 500) == 2 and event_capacity(t[:0], 500) == 0


# ----------------------------------------------------------------------------------------------------------------- on the device

def _device_case(torch, probs, times, thresholds, avg, sup, minc, tally):
    """probs: CUDA tensor or numpy [N, W, 3].  Device trace + events (all, then fired only) against the host class for every head and
    threshold; adds to tally {events, ties}."""
    from multilingual_kws_amd.detector import detect_on_device
    res = detect_on_device(probs, times, thresholds, avg, sup, minc, trace=True)
    fired = detect_on_device(probs, times, thresholds, avg, sup, minc, fired_only=True)
    host = probs.cpu().numpy() if torch.is_tensor(probs) else probs
    N, W = host.shape[:2]
    assert res.counts.shape == (N, len(thresholds)) and res.scores.shape == (N, W) and res.flags.shape == (N, len(thresholds), W)
    events, fired_events = res.events, fired.events
    for n in range(N):
        for k, thr in enumerate(thresholds):
            kw, new, score = _host_steps(host[n], times, thr, avg, sup, minc)
            where = (n, k, avg, sup, minc, W)
            assert _same(res.scores[n], score), where
            assert np.array_equal(res.flags[n, k] & 1, kw.astype(np.uint8)) and np.array_equal((res.flags[n, k] >> 1) & 1, new.astype(np.uint8)), where
            ev = events[n][k]
            idx = np.nonzero(new)[0]
            assert res.counts[n, k] == len(idx) == len(ev), where
            assert np.array_equal(ev["window"], idx) and np.array_equal(ev["fired"], kw[idx].astype(np.int32)) and _same(ev["score"], score[idx]), where
            fv = fired_events[n][k]
            fidx = idx[kw[idx]]
            assert np.array_equal(fv["window"], fidx) and np.all(fv["fired"] == 1) and _same(fv["score"], score[fidx]), where
            tally["events"] += len(idx)
            tally["fires"] += len(fidx)
            tally["ties"] += int(np.sum(score == thr))       # a mean exactly on the threshold (thresholds are never 0.0, the score of a window not evaluated)


def _random_stream(rng, N, W, nan_rows=2):
    """Confidences from a small set of float32 values in runs of random length (so that means land exactly on a threshold), irregular
    and repeated timestamps, a few NaN rows."""
    values = np.array([0, 0.25, 0.5, 0.75, 1, 0.7], np.float32)
    tgt = np.empty((N, W), np.float32)
    for n in range(N):
        runs = values[rng.integers(0, len(values), W)]
        keep = rng.integers(0, 12, W) == 0                       # a new value every ~12 windows
        keep[:1] = True
        tgt[n] = runs[np.maximum.accumulate(np.where(keep, np.arange(W), 0))] if W else runs
    probs = np.stack([1 - tgt, np.zeros_like(tgt), tgt], axis=2).astype(np.float32)
    if W > 8:
        for _ in range(nan_rows):
            probs[rng.integers(0, N), rng.integers(0, W)] = np.nan
    times = np.cumsum(rng.choice([0, 20, 20, 20, 20, 40, 7], W)).astype(np.int64) if W else np.zeros(0, np.int64)
    return probs, times


@pytest.mark.gpu
def test_device_detector_matches_reference_golden_vectors(golden_dir):
    """All 12 cases of detector_golden.json (outputs of the reference's own detector), float64 input, dense trace and events."""
    torch = pytest.importorskip("torch")
    from multilingual_kws_amd.detector import detect_on_device
    G = json.load(open(os.path.join(golden_dir, "detector_golden.json")))
    assert len(G["cases"]) == 12
    steps = n_events = 0
    configs = set()
    for case in G["cases"]:
        cfg = case["config"]
        configs.add((cfg["avg"], cfg["sup"], cfg["minc"], cfg["stride"]))
        probs = np.asarray(case["probs"], np.float64)
        assert probs.shape == (300, 3)
        times = np.arange(300) * cfg["stride"]
        res = detect_on_device(probs[None], times, [cfg["thr"]], cfg["avg"], cfg["sup"], cfg["minc"], trace=True)
        label = np.array([o[0] == "kw" for o in case["outputs"]])
        assert all(o[0] in ("kw", "_silence_") for o in case["outputs"])
        score = np.array([o[1] for o in case["outputs"]], np.float64)
        new = np.array([bool(o[2]) for o in case["outputs"]])
        assert np.array_equal(res.flags[0, 0] & 1, label.astype(np.uint8)), cfg
        assert np.array_equal(res.flags[0, 0] >> 1, new.astype(np.uint8)), cfg
        assert _same(res.scores[0], score), cfg
        ev, idx = res.events[0][0], np.nonzero(new)[0]
        assert res.counts[0, 0] == len(idx) and np.array_equal(ev["window"], idx) and np.array_equal(ev["fired"], label[idx].astype(np.int32))
        assert _same(ev["score"], score[idx]), cfg
        steps += 300
        n_events += len(idx)
    assert steps == 3600 and n_events > 50 and len(configs) == 4
    assert any(s == 0 and m == 1 for _, s, m, _ in configs) and any(st == 40 for _, _, _, st in configs)


@pytest.mark.gpu
def test_device_detector_matches_the_host_class_on_random_streams():
    """float32 input, trace and events, against SingleTargetRecognizeCommands stepped on the host: every average window / suppression /
    minimum count combination, stream lengths that bracket the kernel's 2048-window tile, 70 thresholds (more than one wave), 130
    heads, a non-contiguous view."""
    torch = pytest.importorskip("torch")
    rng = np.random.default_rng(20260)
    tally = dict(events=0, fires=0, ties=0)
    thr3 = [0.25, 0.5, 0.7]
    for avg in (0, 20, 60, 100, 500):
        for sup in (0, 100, 500):
            for minc in (1, 3, 4):
                for W in (0, 1, 3, 4, 5, 90):
                    probs, times = _random_stream(rng, 2, W)
                    _device_case(torch, probs, times, thr3, avg, sup, minc, tally)
    for W, (avg, sup, minc) in zip((2047, 2048, 2049, 5000), ((100, 500, 4), (60, 100, 3), (500, 0, 1), (100, 500, 4))):
        probs, times = _random_stream(rng, 2, W, nan_rows=4)
        _device_case(torch, torch.from_numpy(probs).cuda(), times, thr3, avg, sup, minc, tally)
    # 70 thresholds: lanes of a second wave; repeated and unordered thresholds are lanes like any other
    probs, times = _random_stream(rng, 2, 400)
    thr70 = [thr3[i % 3] if i % 5 == 0 else float(rng.integers(1, 40)) / 40 for i in range(70)]
    _device_case(torch, probs, times, thr70, 100, 100, 3, tally)
    # 130 heads
    probs, times = _random_stream(rng, 130, 300, nan_rows=20)
    _device_case(torch, torch.from_numpy(probs).cuda(), times, thr3, 60, 100, 3, tally)
    # a [N, W, 3] view that is not contiguous: the first three of six columns
    probs, times = _random_stream(rng, 3, 500)
    wide = torch.from_numpy(np.concatenate([probs, np.full_like(probs, 0.9)], axis=2)).cuda()
    view = wide[:, :, :3]
    assert not view.is_contiguous()
    _device_case(torch, view, times, thr3, 100, 500, 4, tally)
    # uniform 20 ms hop, the shipped StreamFlags defaults
    probs, _ = _random_stream(rng, 3, 1500)
    _device_case(torch, probs, np.arange(1500) * 20, thr3, 100, 500, 4, tally)
    print("random streams:", tally)
    assert tally["ties"] >= 1 and tally["events"] > 50 and tally["fires"] > 50, tally     # the inputs did exercise ties and events


def _raw_call(torch, probs, times, thr, avg, sup, minc, cap, d_events, d_counts, fired_only=0):
    from multilingual_kws_amd import _lib
    N, W, C = probs.shape
    return _lib.lib().mkws_detect_stream(probs.data_ptr(), int(probs.dtype == torch.float64), N, W, C, 2, times.data_ptr(), thr.data_ptr(), thr.numel(),
                                         float(avg), float(sup), int(minc), fired_only, d_events.data_ptr(), cap, d_counts.data_ptr(), None, None,
                                         _lib.current_stream_ptr())


@pytest.mark.gpu
def test_event_capacity_cuts_the_list_but_not_the_count():
    """More events than event_cap: the count is the true one, nothing is stored past the cap (neighbouring lanes' lists and guard words
    behind the buffer stay intact); the wrapper's result for the same stream is complete."""
    torch = pytest.importorskip("torch")
    from multilingual_kws_amd import _lib
    from multilingual_kws_amd.detector import EVENT_DTYPE, detect_on_device
    N, W, T, cap, guard = 3, 64, 2, 4, 64
    tgt = np.tile(np.array([1.0, 0.0], np.float32), W // 2)                   # avg 0, minimum_count 1, no suppression: an event per window
    probs = np.stack([np.stack([1 - tgt, 0 * tgt, tgt], 1)] * N)
    probs[1, :, 2] = 0.75                                                       # head 1: one fire at 0.5, never above 0.8
    times = np.arange(W, dtype=np.int64) * 20
    d_probs, d_times = torch.from_numpy(probs).cuda(), torch.from_numpy(times).cuda()
    d_thr = torch.tensor([0.5, 0.8], dtype=torch.float64, device="cuda")
    PATTERN = 0x5A5A5A5A5A5A5A5A
    d_events = torch.full((N * T * cap * 2 + guard,), PATTERN, dtype=torch.int64, device="cuda")
    d_counts = torch.full((N * T + guard,), -7, dtype=torch.int32, device="cuda")
    assert _raw_call(torch, d_probs, d_times, d_thr, 0, 0, 1, cap, d_events, d_counts) == 0
    torch.cuda.synchronize()
    raw, counts = d_events.cpu().numpy(), d_counts.cpu().numpy()
    assert np.all(raw[N * T * cap * 2:] == PATTERN) and np.all(counts[N * T:] == -7)
    counts = counts[:N * T].reshape(N, T)
    ev = raw[:N * T * cap * 2].view(EVENT_DTYPE).reshape(N, T, cap)
    assert counts.tolist() == [[W, W], [1, W], [W, W]]                          # head 1 at 0.8: a release on every window, never a fire
    for n in (0, 2):
        for k in range(T):
            assert ev["window"][n, k].tolist() == [0, 1, 2, 3] and ev["fired"][n, k].tolist() == [1, 0, 1, 0] and ev["score"][n, k].tolist() == [1, 0, 1, 0]
    assert (ev["window"][1, 0, 0], ev["fired"][1, 0, 0], ev["score"][1, 0, 0]) == (0, 1, 0.75)
    assert np.all(raw[(1 * T + 0) * cap * 2 + 2:(1 * T + 1) * cap * 2] == PATTERN)      # the unused rest of a short list is untouched
    # bad arguments are refused, an empty stream is fine and launches nothing
    L = _lib.lib()
    assert _raw_call(torch, d_probs, d_times, d_thr, -1, 0, 1, cap, d_events, d_counts) == -1 and b"average_window_duration_ms" in L.mkws_last_error()
    assert L.mkws_detect_stream(d_probs.data_ptr(), 0, N, W, 3, 3, d_times.data_ptr(), d_thr.data_ptr(), T, 0.0, 0.0, 1, 0, d_events.data_ptr(), cap,
                                d_counts.data_ptr(), None, None, None) == -1
    assert L.mkws_detect_stream(d_probs.data_ptr(), 0, N, W, 3, 2, d_times.data_ptr(), d_thr.data_ptr(), 0, 0.0, 0.0, 1, 0, d_events.data_ptr(), cap,
                                d_counts.data_ptr(), None, None, None) == -1
    assert L.mkws_detect_stream(None, 0, N, W, 3, 2, d_times.data_ptr(), d_thr.data_ptr(), T, 0.0, 0.0, 1, 0, d_events.data_ptr(), cap,
                                d_counts.data_ptr(), None, None, None) == -1
    assert L.mkws_detect_stream(d_probs.data_ptr(), 0, N, 0, 3, 2, d_times.data_ptr(), d_thr.data_ptr(), T, 0.0, 0.0, 1, 0, d_events.data_ptr(), cap,
                                d_counts.data_ptr(), None, None, None) == 0
    # the wrapper: suppression 0 gives capacity W at once; suppression 500 starts from the derived bound and repeats with W
    for sup in (0, 500):
        res = detect_on_device(d_probs, times, [0.5, 0.8], 0, sup, 1)
        for n in range(N):
            for k, thr in enumerate((0.5, 0.8)):
                kw, new, score = _host_steps(probs[n], times, thr, 0, sup, 1)
                e = res.events[n][k]
                assert np.array_equal(e["window"], np.nonzero(new)[0]) and np.array_equal(e["fired"], kw[new].astype(np.int32)) and _same(e["score"], score[new])
        assert res.counts.max() > 2 * (int(times[-1]) // 500) + 2 if sup else res.counts.max() == W


@pytest.mark.gpu
def test_detector_call_is_capturable_in_a_graph():
    """The call recorded in a torch.cuda.graph and replayed on new probabilities gives the eager result."""
    torch = pytest.importorskip("torch")
    from multilingual_kws_amd.detector import EVENT_DTYPE, detect_on_device
    rng = np.random.default_rng(7)
    N, W, T = 5, 2500, 3
    cap = W
    first, times = _random_stream(rng, N, W)
    second, _ = _random_stream(rng, N, W)
    thresholds = [0.25, 0.5, 0.7]
    d_probs = torch.from_numpy(first).cuda()
    d_times = torch.from_numpy(times).cuda()
    d_thr = torch.tensor(thresholds, dtype=torch.float64, device="cuda")
    d_events = torch.zeros((N * T * cap * 2,), dtype=torch.int64, device="cuda")
    d_counts = torch.zeros((N * T,), dtype=torch.int32, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        assert _raw_call(torch, d_probs, d_times, d_thr, 100, 500, 4, cap, d_events, d_counts) == 0
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        assert _raw_call(torch, d_probs, d_times, d_thr, 100, 500, 4, cap, d_events, d_counts) == 0
    for probs in (second, first):
        d_probs.copy_(torch.from_numpy(probs))
        d_events.zero_()
        d_counts.zero_()
        g.replay()
        torch.cuda.synchronize()
        eager = detect_on_device(probs, times, thresholds, 100, 500, 4)
        counts = d_counts.cpu().numpy().reshape(N, T)
        ev = d_events.cpu().numpy().view(EVENT_DTYPE).reshape(N, T, cap)
        assert np.array_equal(counts, eager.counts) and counts.sum() > 50
        for n in range(N):
            for k in range(T):
                a, b = ev[n, k, :counts[n, k]], eager.events[n][k]
                assert np.array_equal(a["window"], b["window"]) and np.array_equal(a["fired"], b["fired"]) and _same(a["score"], b["score"])


@pytest.mark.gpu
def test_detect_many_on_device_tensors_equals_detect():
    """detect_many on CUDA tensors (what streaming_inferences(as_device=True) hands over) = detect() on their host copies."""
    torch = pytest.importorskip("torch")
    n = 400
    flags = sa.StreamFlags(wav="unused.wav", ground_truth="", target_keyword="mask", detection_thresholds=[0.5])
    inf = np.stack([_bursty(n, s, c) for s, c in ((1, [40, 120, 300]), (2, [20, 90]), (3, []))])
    thresholds = [0.5, 0.9, 0.97]
    import dataclasses
    kws = ["a", "b", "c"]
    want = [{t: sa.detect(inf[i], dataclasses.replace(flags, target_keyword=kws[i]), t) for t in thresholds} for i in range(3)]
    assert sum(len(w[0.9][1]) for w in want) == 5
    d = torch.from_numpy(inf).cuda()
    assert sa.detect_many(d, flags, thresholds, keywords=kws) == want
    assert sa.detect_many([d[0], d[1], d[2]], flags, thresholds, keywords=kws) == want
    assert sa.detect_many(d[1], flags, thresholds) == {t: sa.detect(inf[1], flags, t) for t in thresholds}
    assert sa.detect_many(inf, flags, thresholds, keywords=kws) == want             # numpy on a GPU host: uploaded
    assert sa.detect_many(d[:, :0], flags, thresholds, keywords=kws) == [{t: ([], []) for t in thresholds}] * 3
