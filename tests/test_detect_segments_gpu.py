"""mkws_detect_segments / mkws_detect_score_segments and their wrappers (detector.detect_segments_on_device, score_segments_on_device):
S recordings concatenated, each with its own windows, times and probabilities.  The yardstick is the unsegmented call on each slice
alone (detect_on_device / score_on_device, themselves held to the host class in tests/test_detector_device.py), and for the short
segments the host class and tpr_fpr's scans directly.  Every comparison is exact: counts, event records, scores and flags byte for
byte, tallies integer for integer; there is no tolerance to choose."""
import numpy as np
import pytest

from multilingual_kws_amd.embedding.single_target_recognize_commands import RecognizeResult, SingleTargetRecognizeCommands
from multilingual_kws_amd.embedding.tpr_fpr import _in_window_sorted_scan

LENGTHS = [0, 1, 3, 4, 2049, 300]            # empty, shorter than the minimum count, a few windows, one past the 2048-window LDS tile
STARTS = [500, 7, 1000, 90, 12345, 40]       # a start time and a hop of its own for every segment
HOPS = [20, 20, 30, 25, 20, 35]
OFF = np.concatenate([[0], np.cumsum(LENGTHS)]).astype(np.int32)
ROWS = int(OFF[-1])
AVG, SUPPRESSION, MIN_COUNT, TOL = 100, 300, 2, 200
SHORT = (0, 1, 2, 3)
SEED = 11


def _bursty(n, seed, centres, width=8):
    rng = np.random.default_rng(seed)
    tgt = np.full(n, 0.02)
    for c in centres:
        tgt[max(0, c - width):c + width] = 0.97
    other = rng.uniform(0, 1, n) * (1 - tgt)
    return np.stack([1 - tgt - other, other, tgt], axis=1).astype(np.float32)


def _thresholds(n):
    return [0.5] if n == 1 else np.linspace(0.05, 1.0, n).tolist()


@pytest.fixture(scope="module")
def stream():
    centres = [[], [0], [1], [2], [40, 300, 900, 1500, 2046, 2049 - 1], [30, 150, 290]]
    probs = np.concatenate([_bursty(n, SEED + s, centres[s]) for s, n in enumerate(LENGTHS)])
    nan_rows = [int(OFF[4]) + 905, int(OFF[5]) + 152]                     # inside bursts: the averages that include them are NaN
    probs[nan_rows] = np.nan
    times = np.concatenate([STARTS[s] + HOPS[s] * np.arange(n, dtype=np.int64) for s, n in enumerate(LENGTHS)])
    assert times[OFF[4] + 2048] - AVG <= times[OFF[4] + 2047]            # window 2048's average reaches back across the tile boundary
    return dict(probs=probs, times=times, spans=list(zip(OFF[:-1].tolist(), OFF[1:].tolist())), refs={})


def _reference(stream, dtype, n_thr, fired_only):
    """detect_on_device on every slice alone, once per case."""
    from multilingual_kws_amd.detector import detect_on_device
    key = (dtype, n_thr, fired_only)
    if key not in stream["refs"]:
        p = stream["probs"].astype(dtype)
        stream["refs"][key] = [detect_on_device(p[None, a:b], stream["times"][a:b], _thresholds(n_thr), AVG, SUPPRESSION, MIN_COUNT, trace=True,
                                                fired_only=fired_only) for a, b in stream["spans"]]
    return stream["refs"][key]


def _host_walk(probs, times, thr):
    """The host class stepped window by window: (scores, flags, [(window, fired, score)] of the is_new_command steps)."""
    rc, el = SingleTargetRecognizeCommands(["_silence_", "_unknown_", "kw"], AVG, thr, SUPPRESSION, MIN_COUNT, 2), RecognizeResult()
    scores, flags, events = [], [], []
    for w in range(len(times)):
        rc.process_latest_result(probs[w], int(times[w]), el)
        scores.append(el.score)
        flags.append((el.found_command == "kw") + 2 * bool(el.is_new_command))
        if el.is_new_command:
            events.append((w, int(el.found_command == "kw"), el.score))
    return scores, flags, events


@pytest.mark.gpu
@pytest.mark.parametrize("fired_only", [False, True], ids=["all_events", "fired_only"])
@pytest.mark.parametrize("n_thr", [1, 20, 65])
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_every_segment_equals_the_unsegmented_call_on_its_slice(stream, dtype, n_thr, fired_only):
    pytest.importorskip("torch")
    from multilingual_kws_amd.detector import detect_segments_on_device
    thresholds = _thresholds(n_thr)
    got = detect_segments_on_device(stream["probs"].astype(dtype), OFF, stream["times"], thresholds, AVG, SUPPRESSION, MIN_COUNT, trace=True,
                                    fired_only=fired_only)
    refs = _reference(stream, dtype, n_thr, fired_only)
    assert got.counts.shape == (len(LENGTHS), n_thr) and got.counts.dtype == np.int32
    for s, ref in enumerate(refs):
        assert got.counts[s].tolist() == ref.counts[0].tolist(), s
        for k in range(n_thr):
            assert got.events[s][k].tobytes() == ref.events[0][k].tobytes(), (s, k)
        assert got.scores[s].tobytes() == ref.scores[0].tobytes(), s
        assert got.flags[s].tobytes() == ref.flags[0].tobytes() and got.flags[s].shape == (n_thr, LENGTHS[s]), s
    assert got.counts[0].tolist() == [0] * n_thr and got.counts[1].tolist() == [0] * n_thr       # empty / below the minimum count: written, zero
    # the short segments against the host class itself
    for s in SHORT:
        a, b = stream["spans"][s]
        for k in sorted({0, n_thr // 2, n_thr - 1}):
            scores, flags, events = _host_walk(stream["probs"].astype(dtype)[a:b], stream["times"][a:b], thresholds[k])
            assert got.scores[s].tolist() == scores and got.flags[s][k].tolist() == flags, (s, k)
            assert [tuple(e) for e in got.events[s][k].tolist()] == [e for e in events if e[1] or not fired_only], (s, k)
    # not vacuous: a lane that fires repeatedly, a lane that never does, and a lookback across the tile boundary that is evaluated
    fires = np.array([[int(got.events[s][k]["fired"].sum()) for k in range(n_thr)] for s in range(len(LENGTHS))])
    assert fires[4].max() >= 2 and fires[2:4].max() >= 1 and (fires[4:] == 0).any() == (n_thr > 1)
    assert got.scores[4][2048] > 0.5 and got.flags[4][0, 2040:2049].any()
    assert np.isnan(got.scores[4][905]) and np.isnan(got.scores[5][152])


def _raw_detect(torch, probs, times, thresholds, cap, fired_only, tail=0):
    """The C call itself with an event capacity of the caller's choosing; `tail` canary records behind the event buffer."""
    from multilingual_kws_amd import _lib
    S, T = len(LENGTHS), len(thresholds)
    d = dict(probs=torch.from_numpy(probs).cuda(), times=torch.from_numpy(times).cuda(), off=torch.from_numpy(OFF).cuda(),
             thr=torch.tensor(thresholds, dtype=torch.float64, device="cuda"),
             events=torch.full((2 * (S * T * cap + tail),), -77, dtype=torch.int64, device="cuda"),
             counts=torch.full((S * T,), -5, dtype=torch.int32, device="cuda"))
    code = _lib.lib().mkws_detect_segments(d["probs"].data_ptr(), int(probs.dtype == np.float64), d["off"].data_ptr(), S, ROWS, 3, 2, d["times"].data_ptr(),
                                           d["thr"].data_ptr(), T, float(AVG), float(SUPPRESSION), MIN_COUNT, int(fired_only), d["events"].data_ptr(), cap,
                                           d["counts"].data_ptr(), None, None, _lib.current_stream_ptr())
    torch.cuda.synchronize()
    return code, d


@pytest.mark.gpu
def test_a_capacity_below_a_lanes_count_cuts_the_list_and_stores_nothing_past_it(stream):
    torch = pytest.importorskip("torch")
    from multilingual_kws_amd.detector import EVENT_DTYPE
    thresholds = _thresholds(20)
    full = _reference(stream, np.float32, 20, False)
    cap, tail = 2, 4
    code, d = _raw_detect(torch, stream["probs"], stream["times"], thresholds, cap, False, tail=tail)
    assert code == 0
    counts = d["counts"].cpu().numpy().reshape(len(LENGTHS), 20)
    events = d["events"].cpu().numpy()
    lanes = events[:2 * len(LENGTHS) * 20 * cap].view(EVENT_DTYPE).reshape(len(LENGTHS), 20, cap)
    assert (events[2 * len(LENGTHS) * 20 * cap:] == -77).all()                                   # the canary behind the buffer
    for s, ref in enumerate(full):
        assert counts[s].tolist() == ref.counts[0].tolist()                                     # what OCCURRED, not what was stored
        for k in range(20):
            kept = min(cap, int(counts[s, k]))
            assert lanes[s, k, :kept].tobytes() == ref.events[0][k][:kept].tobytes()
            assert (lanes[s, k, kept:].view(np.int64) == -77).all()                             # slots past a lane's count are not written
    assert counts.max() > cap


def _raw_tally(found_times, gt, tol):
    return [len(found_times), sum(_in_window_sorted_scan(gt, t, tol) for t in found_times),
            sum(not _in_window_sorted_scan(found_times, g, tol) for g in gt)]


def _groundtruth(stream):
    t = stream["times"]
    seg = [t[a:b] for a, b in stream["spans"]]
    return [
        [100.0, 5.0],                                                    # an empty segment still has occurrences to miss
        [],
        [float(seg[2][2]) + 150.0, float(seg[2][0])],                    # unsorted
        [float(x) for x in seg[3]],
        [float(x) for x in np.linspace(seg[4][0], seg[4][-1], 2049)],    # one past the 2048-entry LDS stage
        [float(seg[5][150]) + 180.0, float(seg[5][30]), 9.0e6, float(seg[5][290]) - 190.0],   # unsorted, with a decoy
    ]


@pytest.mark.gpu
@pytest.mark.parametrize("n_thr", [1, 20, 65])
def test_tallies_equal_the_unsegmented_scorer_per_slice_and_the_host_scans(stream, n_thr):
    pytest.importorskip("torch")
    from multilingual_kws_amd.detector import score_on_device, score_segments_on_device
    thresholds, gt = _thresholds(n_thr), _groundtruth(stream)
    assert len(gt[4]) == 2049 and gt[2] != sorted(gt[2]) and gt[5] != sorted(gt[5])
    got = score_segments_on_device(stream["probs"], OFF, stream["times"], thresholds, gt, TOL, AVG, SUPPRESSION, MIN_COUNT)
    assert got.shape == (len(LENGTHS), n_thr, 3) and got.dtype == np.int32
    for s, (a, b) in enumerate(stream["spans"]):
        if a == b:                                                       # (the unsegmented call takes no stream without windows: asserted below)
            continue
        want = score_on_device(stream["probs"][None, a:b], stream["times"][a:b], thresholds, [gt[s]], TOL, AVG, SUPPRESSION, MIN_COUNT)
        assert got[s].tolist() == want[0].tolist(), s
    assert got[0].tolist() == [[0, 0, 2]] * n_thr and got[1].tolist() == [[0, 0, 0]] * n_thr       # {0, 0, entries}
    assert got[4, 0, 0] >= 4 and got[4, 0, 1] >= 4 and got[4, 0, 2] > 1000 and got[5, 0, 2] >= 1
    for s in SHORT:                                                      # tpr_fpr's scans on the host class's fires
        a, b = stream["spans"][s]
        for k in sorted({0, n_thr // 2, n_thr - 1}):
            events = _host_walk(stream["probs"][a:b], stream["times"][a:b], thresholds[k])[2]
            found = [int(stream["times"][a + w]) for w, fired, _ in events if fired]
            assert got[s, k].tolist() == _raw_tally(found, gt[s], TOL), (s, k)
    assert got[3, 0].tolist()[0] >= 1 and got[3, 0].tolist()[1] >= 1


@pytest.mark.gpu
def test_a_cut_lane_is_flagged_alone_and_the_wrapper_raises(stream, monkeypatch):
    torch = pytest.importorskip("torch")
    from multilingual_kws_amd import _lib, detector
    thresholds, gt = _thresholds(20), _groundtruth(stream)
    whole = detector.score_segments_on_device(stream["probs"], OFF, stream["times"], thresholds, gt, TOL, AVG, SUPPRESSION, MIN_COUNT)
    cap = 2
    code, d = _raw_detect(torch, stream["probs"], stream["times"], thresholds, cap, True)
    assert code == 0
    values, offsets = detector.pack_groundtruth(gt, len(LENGTHS))
    d_gt, d_gt_off = torch.from_numpy(values).cuda(), torch.from_numpy(offsets).cuda()
    d_tally = torch.full((len(LENGTHS), 20, 4), -9, dtype=torch.int32, device="cuda")
    assert _lib.lib().mkws_detect_score_segments(d["events"].data_ptr(), d["counts"].data_ptr(), d["off"].data_ptr(), len(LENGTHS), ROWS, 20, cap,
                                                 d["times"].data_ptr(), d_gt.data_ptr(), d_gt_off.data_ptr(), float(TOL), d_tally.data_ptr(),
                                                 _lib.current_stream_ptr()) == 0
    tally = d_tally.cpu().numpy()
    cut = whole[:, :, 0] > cap
    assert cut.any() and not cut.all() and cut[4].any() and (whole[~cut][:, 0] > 0).any()
    assert (tally[:, :, 3] == cut).all()                                 # flagged: exactly the lanes whose list is incomplete
    assert (tally[:, :, 0] == whole[:, :, 0]).all()                      # `found` is the count either way
    assert (tally[~cut][:, :3] == whole[~cut]).all()                     # their neighbours are scored as before
    monkeypatch.setattr(detector, "event_capacity", lambda times, suppression_ms, fired_only=False: min(len(times), cap))
    with pytest.raises(RuntimeError, match="the list was cut"):
        detector.score_segments_on_device(stream["probs"], OFF, stream["times"], thresholds, gt, TOL, AVG, SUPPRESSION, MIN_COUNT)
    # the detector wrapper itself never returns a cut list: it repeats the call at the longest segment's length
    res = detector.detect_segments_on_device(stream["probs"], OFF, stream["times"], thresholds, AVG, SUPPRESSION, MIN_COUNT, fired_only=True)
    assert res.event_buffer.shape[2] == max(LENGTHS) and (res.counts == whole[:, :, 0]).all()


@pytest.mark.gpu
def test_detector_and_scorer_are_captured_as_one_chain(stream):
    torch = pytest.importorskip("torch")
    from multilingual_kws_amd import _lib
    from multilingual_kws_amd.detector import event_capacity, pack_groundtruth, score_segments_on_device
    L = _lib.lib()
    S, T = len(LENGTHS), 20
    thresholds, gt = _thresholds(T), _groundtruth(stream)
    first = stream["probs"]
    second = np.concatenate([first[OFF[4]:OFF[5]][::-1], first[:OFF[4]], first[OFF[5]:]])          # other numbers in the same shape
    cap = max(event_capacity(stream["times"][a:b], SUPPRESSION, True) for a, b in stream["spans"])
    d_probs = torch.from_numpy(first).cuda()
    d_times, d_off = torch.from_numpy(stream["times"]).cuda(), torch.from_numpy(OFF).cuda()
    d_thr = torch.tensor(thresholds, dtype=torch.float64, device="cuda")
    values, offsets = pack_groundtruth(gt, S)
    d_gt, d_gt_off = torch.from_numpy(values).cuda(), torch.from_numpy(offsets).cuda()
    d_events = torch.empty(2 * S * T * cap, dtype=torch.int64, device="cuda")
    d_counts = torch.empty(S * T, dtype=torch.int32, device="cuda")
    d_tally = torch.zeros((S, T, 4), dtype=torch.int32, device="cuda")

    def chain():
        s = _lib.current_stream_ptr()
        assert L.mkws_detect_segments(d_probs.data_ptr(), 0, d_off.data_ptr(), S, ROWS, 3, 2, d_times.data_ptr(), d_thr.data_ptr(), T, float(AVG),
                                      float(SUPPRESSION), MIN_COUNT, 1, d_events.data_ptr(), cap, d_counts.data_ptr(), None, None, s) == 0
        assert L.mkws_detect_score_segments(d_events.data_ptr(), d_counts.data_ptr(), d_off.data_ptr(), S, ROWS, T, cap, d_times.data_ptr(), d_gt.data_ptr(),
                                            d_gt_off.data_ptr(), float(TOL), d_tally.data_ptr(), s) == 0
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        chain()
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        chain()
    seen = []
    for probs in (second, first):
        d_probs.copy_(torch.from_numpy(probs))
        d_tally.zero_()
        g.replay()
        torch.cuda.synchronize()
        got = d_tally.cpu().numpy()
        assert np.array_equal(got[:, :, :3], score_segments_on_device(probs, OFF, stream["times"], thresholds, gt, TOL, AVG, SUPPRESSION, MIN_COUNT))
        assert not got[:, :, 3].any()
        seen.append(got)
    assert not np.array_equal(seen[0], seen[1]) and seen[1][:, :, 0].sum() > 20


@pytest.mark.gpu
def test_argument_checks_and_empty_calls():
    torch = pytest.importorskip("torch")
    from multilingual_kws_amd import _lib
    from multilingual_kws_amd.detector import detect_segments_on_device, score_segments_on_device
    L, s = _lib.lib(), _lib.current_stream_ptr()
    buf = torch.zeros(64, dtype=torch.int64, device="cuda")
    p = buf.data_ptr()
    assert L.mkws_detect_segments(p, 0, p, 0, 0, 3, 2, p, p, 1, 100.0, 500.0, 4, 1, p, 1, p, None, None, s) == 0            # n_seg == 0: nothing launched
    assert L.mkws_detect_segments(p, 0, p, 1, 0, 3, 2, p, p, 0, 100.0, 500.0, 4, 1, p, 1, p, None, None, s) == -1           # no threshold
    assert L.mkws_detect_segments(p, 0, p, 1, 0, 3, 3, p, p, 1, 100.0, 500.0, 4, 1, p, 1, p, None, None, s) == -1           # target outside the classes
    assert L.mkws_detect_segments(p, 0, p, 1, 0, 3, 2, p, p, 1, -1.0, 500.0, 4, 1, p, 1, p, None, None, s) == -1            # negative average window
    assert L.mkws_detect_segments(p, 0, None, 1, 0, 3, 2, p, p, 1, 100.0, 500.0, 4, 1, p, 1, p, None, None, s) == -1        # no offsets
    assert L.mkws_detect_segments(None, 0, p, 1, 4, 3, 2, p, p, 1, 100.0, 500.0, 4, 1, p, 1, p, None, None, s) == -1        # rows but no probabilities
    assert L.mkws_detect_score_segments(p, p, p, 0, 0, 1, 1, p, p, p, 750.0, p, s) == 0
    assert L.mkws_detect_score_segments(p, p, p, 1, 0, 1, 1, p, p, p, -1.0, p, s) == -1
    assert L.mkws_detect_score_segments(p, p, None, 1, 0, 1, 1, p, p, p, 750.0, p, s) == -1
    # every segment empty: counts are still written, and scored
    res = detect_segments_on_device(np.zeros((0, 3), np.float32), [0, 0, 0], [], [0.5, 0.7], 100, 500, 4, trace=True)
    assert res.counts.tolist() == [[0, 0], [0, 0]] and res.event_buffer.shape == (2, 2, 0) and [x.shape for x in res.flags] == [(2, 0), (2, 0)]
    assert score_segments_on_device(np.zeros((0, 3), np.float32), [0, 0, 0], [], [0.5, 0.7], [[1.0, 2.0], []], 750, 100, 500, 4).tolist() == \
        [[[0, 0, 2], [0, 0, 2]], [[0, 0, 0], [0, 0, 0]]]
    assert detect_segments_on_device(np.zeros((0, 3), np.float32), [0], [], [0.5], 100, 500, 4).counts.shape == (0, 1)
