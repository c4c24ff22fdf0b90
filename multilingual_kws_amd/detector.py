"""Device streaming detector: host wrappers over mkws_detect_stream / mkws_detect_segments and their scorers (include/mkws.h).

SingleTargetRecognizeCommands (embedding/single_target_recognize_commands.py) stepped over every window of a stream, for P planes x T
detection thresholds in one launch.  A plane is one walk of the detector: a keyword head over the windows of ONE recording
(detect_on_device) or one of S recordings laid back to back, each with its own windows and times (detect_segments_on_device).  The host
class is the specification: labels, is_new_command and the float64 scores are equal bit for bit (tests/test_detector_device.py).
score_on_device / score_segments_on_device go on to mkws_detect_score[_segments]: the fires of every lane matched against ground-truth
times on the device, embedding/tpr_fpr.py being the specification (tests/test_operating_curve_gpu.py).

The four entry points keep what differs between the two forms (how the times are checked, the C call, the event capacity and its
fallback, the per-plane views of trace output, the empty returns) and share the rest: _check_thresholds, _check_tolerance,
_device_probs, and the device rounds _detect_round and _score_round, each one upload, one device-to-host copy, one synchronisation."""
import ctypes

import numpy as np

from . import _lib

# mkws_detect_event as a numpy record (the layout of _lib.DetectEvent)
EVENT_DTYPE = np.dtype([("window", "<i4"), ("fired", "<i4"), ("score", "<f8")])
assert EVENT_DTYPE.itemsize == ctypes.sizeof(_lib.DetectEvent) == 16


class DetectResult:
    """counts int32 [N, T]; events[n][k]: EVENT_DTYPE records of head n at thresholds[k], in window order (views of `event_buffer`
    [N, T, cap]); with trace=True scores float64 [N, W] (0.0 where the window was not evaluated) and flags uint8 [N, T, W] (bit 0
    found_command is the keyword, bit 1 is_new_command), else None."""

    def __init__(self, counts, event_buffer, scores=None, flags=None):
        self.counts, self.event_buffer, self.scores, self.flags = counts, event_buffer, scores, flags

    @property
    def events(self):
        return [[self.event_buffer[n, k, :c] for k, c in enumerate(row)] for n, row in enumerate(self.counts.tolist())]


def check_times(times_ms):
    """int64 [W], non-decreasing -- with the ValueError of SingleTargetRecognizeCommands.process_latest_result (which compares a new
    timestamp with the oldest one it still holds; here the whole list is known up front, so any step backwards is refused)."""
    t = np.asarray(times_ms)
    if t.ndim != 1 or (t.size and not np.issubdtype(t.dtype, np.integer) and not np.array_equal(t, np.floor(t))):
        raise ValueError("times_ms must be a one-dimensional list of integer milliseconds")
    t = np.ascontiguousarray(t, dtype=np.int64)
    if t.size and max(abs(int(t[0])), abs(int(t[-1]))) > 2 ** 61:
        raise ValueError("times_ms must lie within +-2**61 milliseconds")
    bad = np.nonzero(t[1:] < t[:-1])[0]
    if bad.size:
        i = int(bad[0])
        raise ValueError("Results must be fed in increasing time order, but receive a timestamp of {}, which was "
                         "earlier than the previous one of {}".format(int(t[i + 1]), int(t[i])))
    return t


def event_capacity(times_ms, suppression_ms, fired_only=False):
    """Upper bound on the events of one (head, threshold) lane that leave or enter the keyword state.  A release out of the keyword
    state needs more than suppression_ms since the fire, but a fire may follow a release in the very next window (the class takes
    `since` as infinite while the label is silence): at most two such events per suppression_ms of stream.  Fires alone are more than
    suppression_ms apart.  (With fired_only=False the class's repeated releases of an already silent label count as events too and can
    exceed this: detect_on_device then repeats the call with capacity W.)"""
    W = len(times_ms)
    if W == 0:
        return 0
    if not suppression_ms > 0 or not np.isfinite(suppression_ms):
        return W
    per = int((int(times_ms[-1]) - int(times_ms[0])) // suppression_ms)
    return min(W, per + 2 if fired_only else 2 * per + 2)


def _check_thresholds(thresholds, average_window_duration_ms):
    """-> float64 [T], T >= 1."""
    thr = np.ascontiguousarray(np.asarray(thresholds, dtype=np.float64).reshape(-1))
    if thr.size < 1:
        raise ValueError("at least one threshold")
    if not average_window_duration_ms >= 0:
        raise ValueError("average_window_duration_ms must be >= 0")
    return thr


def _check_tolerance(time_tolerance_ms, span):
    """-> the tolerance as a float; span: the largest |time| of the call."""
    tol = float(time_tolerance_ms)
    if not tol >= 0:
        raise ValueError("time_tolerance_ms must be >= 0")
    # the device forms t +- tol in float64; CPython does so too for a float tolerance and exactly for an int one: the same while both fit 2^53
    if span > 2 ** 53 or (np.isfinite(tol) and span + tol > 2 ** 53):
        raise ValueError("times_ms (and times_ms +- time_tolerance_ms) must lie within +-2**53 milliseconds: they are compared as float64")
    return tol


def _device_probs(probs, rank, shape_text, n_times, mismatch, target_id):
    """probs as the C calls read them: a contiguous CUDA tensor of `rank` dimensions [..., rows, classes], float32 or float64, with one
    row per timestamp (`mismatch`: the message for another count, formatted with the two) and target_id among its classes.  A numpy
    array is uploaded."""
    import torch
    if not torch.is_tensor(probs):
        a = np.asarray(probs)
        probs = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64 if a.dtype == np.float64 else np.float32)).cuda()
    if probs.dim() != rank or not probs.is_cuda or probs.dtype not in (torch.float32, torch.float64):
        raise ValueError(f"probs must be a CUDA tensor or numpy array {shape_text} of float32 or float64")
    rows, C = probs.shape[-2:]
    if rows != n_times:
        raise ValueError(mismatch.format(rows, n_times))
    if not 0 <= int(target_id) < C:
        raise ValueError(f"target_id {target_id} outside [0, {C})")
    return probs.contiguous()


def _detect_round(probs, parts, launch, P, T, cap, most, fired_only, trace_rows):
    """The detector over P planes x T thresholds with its events on the host.  parts: what the launch reads beside probs, one upload;
    launch(L, pointers of the parts, fired_only, events, cap, counts, scores, flags, stream): the form's C call.  -> (counts int32 [P, T],
    events EVENT_DTYPE [P, T, capacity], scores float64 [trace_rows] and flags uint8 [T * trace_rows] as the kernel lays them out, or None
    for trace_rows=None).  One launch and one copy (= one synchronisation); a second round at capacity `most` if a lane had more than
    `cap` events."""
    import torch
    L = _lib.lib()
    dev = probs.device
    trace = trace_rows is not None
    with torch.cuda.device(dev):
        d_in, ptrs = _lib.upload_words(parts, dev)
        d_scores = torch.empty(trace_rows, dtype=torch.float64, device=dev) if trace else None
        d_flags = torch.empty(T * trace_rows, dtype=torch.uint8, device=dev) if trace else None
        while True:
            # counts (int32 pairs padded to whole 8-byte words) and events in ONE buffer, so that they cross in one copy
            cwords = (P * T + 1) // 2
            d_out = torch.empty(cwords + 2 * P * T * cap, dtype=torch.int64, device=dev)
            base = d_out.data_ptr()
            _lib.check(launch(L, ptrs, int(bool(fired_only)), base + 8 * cwords, cap, base, d_scores.data_ptr() if trace else None,
                              d_flags.data_ptr() if trace else None, _lib.current_stream_ptr()))
            out = d_out.cpu().numpy()                                  # the call's one synchronisation
            counts = out[:cwords].view(np.int32)[:P * T].reshape(P, T)
            if int(counts.max()) <= cap:
                break
            cap = most
        events = out[cwords:].view(EVENT_DTYPE).reshape(P, T, cap)
        return counts, events, d_scores.cpu().numpy() if trace else None, d_flags.cpu().numpy() if trace else None


def _score_round(probs, parts, launch, launch_score, P, T, cap, noun):
    """The fires of P planes x T thresholds matched against ground truth without leaving the device: parts and launch as _detect_round,
    launch_score(L, pointers of the parts, events, counts, cap, tally, stream): the form's scorer.  -> int32 [P, T, 3].  One upload, two
    launches, one copy of 16 bytes per lane (= one synchronisation); RuntimeError naming the `noun` ("head", "segment") of a lane whose
    event list was cut."""
    import torch
    L = _lib.lib()
    dev = probs.device
    with torch.cuda.device(dev):
        d_in, ptrs = _lib.upload_words(parts, dev)
        d_events = torch.empty(2 * P * T * cap, dtype=torch.int64, device=dev)
        d_counts = torch.empty(P * T, dtype=torch.int32, device=dev)
        d_tally = torch.empty((P, T, 4), dtype=torch.int32, device=dev)
        stream = _lib.current_stream_ptr()
        _lib.check(launch(L, ptrs, 1, d_events.data_ptr(), cap, d_counts.data_ptr(), None, None, stream))
        _lib.check(launch_score(L, ptrs, d_events.data_ptr(), d_counts.data_ptr(), cap, d_tally.data_ptr(), stream))
        tally = d_tally.cpu().numpy()                                  # the call's one synchronisation: 16 bytes per lane
    if tally[:, :, 3].any():
        n, k = (int(x[0]) for x in np.nonzero(tally[:, :, 3]))
        raise RuntimeError(f"{noun} {n}, threshold {k}: {int(tally[n, k, 0])} fires for an event list of {cap}; the list was cut and cannot be scored")
    return np.ascontiguousarray(tally[:, :, :3])


def _stream_form(probs, times, T, average_window_duration_ms, suppression_ms, minimum_count, target_id):
    """The head form: -> (probs [N, W, C] as checked by _device_probs, the `launch` of the two rounds = mkws_detect_stream, for parts that
    begin with times and thresholds)."""
    import torch
    probs = _device_probs(probs, 3, "[heads, windows, classes]", times.shape[0], "{} windows but {} timestamps", target_id)
    N, W, C = probs.shape
    return probs, lambda L, ptrs, *out: L.mkws_detect_stream(
        probs.data_ptr(), int(probs.dtype == torch.float64), N, W, C, int(target_id), ptrs[0], ptrs[1], T,
        float(average_window_duration_ms), float(suppression_ms), int(minimum_count), *out)


def detect_on_device(probs, times_ms, thresholds, average_window_duration_ms, suppression_ms, minimum_count, target_id=2, trace=False,
                     fired_only=False):
    """probs: CUDA tensor [N, W, C], float32 or float64 (made contiguous if it is a view), or a numpy array, which is uploaded.
    times_ms: W non-decreasing integers.  thresholds: T floats.  -> DetectResult; never a cut event list.  One upload (times and
    thresholds), one launch and one device-to-host copy (= one synchronisation) per call; a second round only if a lane had more events
    than event_capacity() allows for (fired_only=False on a stream with quiet stretches)."""
    times = check_times(times_ms)                                      # before anything touches the device
    thr = _check_thresholds(thresholds, average_window_duration_ms)
    T = int(thr.size)
    probs, launch = _stream_form(probs, times, T, average_window_duration_ms, suppression_ms, minimum_count, target_id)
    N, W, _ = probs.shape
    if N == 0 or W == 0:                                               # nothing to launch (the C call would write nothing either)
        return DetectResult(np.zeros((N, T), np.int32), np.zeros((N, T, 0), EVENT_DTYPE),
                            np.zeros((N, W), np.float64) if trace else None, np.zeros((N, T, W), np.uint8) if trace else None)
    # a lane cannot have more events than windows
    counts, events, scores, flags = _detect_round(probs, [times, thr], launch, N, T, event_capacity(times, suppression_ms, fired_only), W,
                                                  fired_only, N * W if trace else None)
    return DetectResult(counts, events, scores.reshape(N, W) if trace else None, flags.reshape(N, T, W) if trace else None)


SCORE_GT_TILE = 2048      # ground-truth entries of a head the score kernel stages in LDS at a time (kScoreTile, csrc/mkws_detect.hip)


def pack_groundtruth(gt_times_per_head, n_heads):
    """Per-head lists of ground-truth times (any order, may be empty) -> (float64 values back to back, int32 offsets [n_heads + 1])."""
    lists = [np.asarray(g, dtype=np.float64).reshape(-1) for g in gt_times_per_head]
    if len(lists) != n_heads:
        raise ValueError(f"{len(lists)} ground-truth lists for {n_heads} heads")
    values = np.concatenate(lists) if lists else np.zeros(0, np.float64)
    if not np.all(np.isfinite(values)):
        raise ValueError("ground-truth times must be finite")
    if values.size >= 2 ** 31:
        raise ValueError("too many ground-truth entries")
    offsets = np.zeros(n_heads + 1, np.int32)
    np.cumsum([g.size for g in lists], out=offsets[1:])
    return np.ascontiguousarray(values), offsets


def score_on_device(probs, times_ms, thresholds, gt_times_per_head, time_tolerance_ms, average_window_duration_ms, suppression_ms, minimum_count,
                    target_id=2):
    """The fires of N heads x T thresholds (detect_on_device(..., fired_only=True)) matched against each head's ground-truth times on the
    device (mkws_detect_score): -> int32 [N, T, 3] = (found, true_positives_raw, false_negatives) per lane, the three integers
    embedding/tpr_fpr.tpr_fpr derives everything from (true_positives_raw is not yet capped to the number of occurrences).  probs,
    times_ms, thresholds as detect_on_device; gt_times_per_head: N lists of times in ms, in the order tpr_fpr would be given them.
    One upload (times, thresholds, ground truth, offsets), two launches, one copy of 16 * N * T bytes (= one synchronisation): no event
    list reaches the host; RuntimeError if a lane's event list was cut."""
    times = check_times(times_ms)
    thr = _check_thresholds(thresholds, average_window_duration_ms)
    tol = _check_tolerance(time_tolerance_ms, max(abs(int(times[0])), abs(int(times[-1]))) if times.size else 0)   # (non-decreasing)
    gt, gt_off = pack_groundtruth(gt_times_per_head, len(probs))        # refused before anything is uploaded
    T = int(thr.size)
    probs, launch = _stream_form(probs, times, T, average_window_duration_ms, suppression_ms, minimum_count, target_id)
    N, W, _ = probs.shape
    if N == 0:
        return np.zeros((0, T, 3), np.int32)
    return _score_round(probs, [times, thr, gt, gt_off], launch,
                        lambda L, ptrs, events, counts, cap, tally, stream: L.mkws_detect_score(
                            events, counts, N, T, cap, ptrs[0], W, ptrs[2], ptrs[3], tol, tally, stream),
                        N, T, event_capacity(times, suppression_ms, fired_only=True), "head")


# ---------------------------------------------------------------------------------------------------------------------------------
# Segmented forms (mkws_detect_segments / mkws_detect_score_segments): S recordings concatenated, each with its own windows, times and
# probabilities -- K (keyword, recording) pairs in one launch where detect_on_device takes N heads over ONE recording.


def check_segments(seg_offsets, times_ms):
    """seg_offsets: S + 1 non-decreasing integers from 0 to len(times_ms); times_ms: the segments' times back to back, non-decreasing
    inside each segment (check_times per segment, with its ValueError).  -> (int32 offsets [S + 1], int64 times [rows]); ValueError
    before anything touches a device."""
    off = np.asarray(seg_offsets)
    if off.ndim != 1 or off.size < 1 or (not np.issubdtype(off.dtype, np.integer) and not np.array_equal(off, np.floor(off))):
        raise ValueError("seg_offsets must be a one-dimensional list of S + 1 integers")
    off = off.astype(np.int64)
    if np.any(off[1:] < off[:-1]):
        s = int(np.nonzero(off[1:] < off[:-1])[0][0])
        raise ValueError(f"seg_offsets must be non-decreasing, but segment {s} runs from {int(off[s])} to {int(off[s + 1])}")
    t = np.asarray(times_ms)
    if t.ndim != 1:
        raise ValueError("times_ms must be a one-dimensional list of integer milliseconds")
    if int(off[0]) != 0 or int(off[-1]) != t.shape[0]:
        raise ValueError(f"seg_offsets run from {int(off[0])} to {int(off[-1])} for {t.shape[0]} timestamps: they must cover exactly [0, rows]")
    if t.shape[0] >= 2 ** 31:
        raise ValueError("too many rows")
    parts = [check_times(t[a:b]) for a, b in zip(off[:-1].tolist(), off[1:].tolist())]
    times = np.concatenate(parts) if parts else np.zeros(0, np.int64)
    return off.astype(np.int32), np.ascontiguousarray(times, dtype=np.int64)


class SegmentDetectResult(DetectResult):
    """DetectResult over S segments: counts int32 [S, T]; events[s][k] in window order, `window` being the index inside segment s; with
    trace=True scores is a list of S float64 [len_s] and flags a list of S uint8 [T, len_s], else None."""


def _segment_capacity(times, spans, suppression_ms, fired_only):
    """The largest event_capacity over the segments, and the longest segment."""
    return (max([event_capacity(times[a:b], suppression_ms, fired_only) for a, b in spans], default=0),
            max([b - a for a, b in spans], default=0))


def _segments_form(probs, times, S, T, average_window_duration_ms, suppression_ms, minimum_count, target_id):
    """The segmented form: -> (probs [R, C] as checked by _device_probs, the `launch` of the two rounds = mkws_detect_segments, for parts
    that begin with times, thresholds and segment offsets)."""
    import torch
    probs = _device_probs(probs, 2, "[rows, classes]", times.shape[0], "{} rows of probabilities but {} timestamps", target_id)
    R, C = probs.shape
    return probs, lambda L, ptrs, *out: L.mkws_detect_segments(
        probs.data_ptr(), int(probs.dtype == torch.float64), ptrs[2], S, R, C, int(target_id), ptrs[0], ptrs[1], T,
        float(average_window_duration_ms), float(suppression_ms), int(minimum_count), *out)


def detect_segments_on_device(probs, seg_offsets, times_ms, thresholds, average_window_duration_ms, suppression_ms, minimum_count, target_id=2,
                              trace=False, fired_only=False):
    """detect_on_device for S concatenated recordings: probs CUDA tensor (or numpy array, which is uploaded) [rows, C], float32 or
    float64; segment s = rows seg_offsets[s] .. seg_offsets[s + 1] with its own non-decreasing times_ms[those rows]; thresholds: T
    floats.  -> SegmentDetectResult whose segment s equals detect_on_device on that slice alone; never a cut event list.  One upload
    (times, thresholds and offsets), one launch and one device-to-host copy (= one synchronisation) per call; a second round at the
    longest segment's length only if a lane had more events than the largest event_capacity() over the segments allows for."""
    off, times = check_segments(seg_offsets, times_ms)                 # before anything touches the device
    thr = _check_thresholds(thresholds, average_window_duration_ms)
    S, T = int(off.shape[0]) - 1, int(thr.size)
    probs, launch = _segments_form(probs, times, S, T, average_window_duration_ms, suppression_ms, minimum_count, target_id)
    if S == 0:
        return SegmentDetectResult(np.zeros((0, T), np.int32), np.zeros((0, T, 0), EVENT_DTYPE), [] if trace else None, [] if trace else None)
    spans = list(zip(off[:-1].tolist(), off[1:].tolist()))
    # a lane cannot have more events than its segment has windows
    cap, longest = _segment_capacity(times, spans, suppression_ms, fired_only)
    counts, events, scores, flags = _detect_round(probs, [times, thr, off], launch, S, T, cap, longest, fired_only,
                                                  times.shape[0] if trace else None)
    if trace:
        scores, flags = [scores[a:b] for a, b in spans], [flags[T * a:T * b].reshape(T, b - a) for a, b in spans]
    return SegmentDetectResult(counts, events, scores, flags)


def score_segments_on_device(probs, seg_offsets, times_ms, thresholds, gt_times_per_segment, time_tolerance_ms, average_window_duration_ms,
                             suppression_ms, minimum_count, target_id=2):
    """score_on_device for S concatenated recordings (mkws_detect_segments + mkws_detect_score_segments): -> int32 [S, T, 3] = (found,
    true_positives_raw, false_negatives) per (segment, threshold) lane; segment s equals score_on_device on that slice with
    gt_times_per_segment[s].  One upload, two launches, one copy of 16 * S * T bytes (= one synchronisation); RuntimeError if a lane's
    event list was cut."""
    off, times = check_segments(seg_offsets, times_ms)
    thr = _check_thresholds(thresholds, average_window_duration_ms)
    tol = _check_tolerance(time_tolerance_ms, int(np.abs(times).max()) if times.size else 0)
    S, T = int(off.shape[0]) - 1, int(thr.size)
    gt, gt_off = pack_groundtruth(gt_times_per_segment, S)             # refused before anything is uploaded
    probs, launch = _segments_form(probs, times, S, T, average_window_duration_ms, suppression_ms, minimum_count, target_id)
    if S == 0:
        return np.zeros((0, T, 3), np.int32)
    R = int(times.shape[0])
    spans = list(zip(off[:-1].tolist(), off[1:].tolist()))
    return _score_round(probs, [times, thr, off, gt, gt_off], launch,
                        lambda L, ptrs, events, counts, cap, tally, stream: L.mkws_detect_score_segments(
                            events, counts, ptrs[2], S, R, T, cap, ptrs[0], ptrs[3], ptrs[4], tol, tally, stream),
                        S, T, _segment_capacity(times, spans, suppression_ms, True)[0], "segment")


# ---------------------------------------------------------------------------------------------------------------------------------
# Live form (mkws_detect_live_step): the detector stepped over the few windows a push completed, its state in a device block of the
# caller's.  LiveDetectorHost is the host restatement -- the specification, and what runs without a GPU.

LIVE_MAX_HISTORY = 256    # MKWS_DETECT_LIVE_MAX_HISTORY
LIVE_MAX_NEW = 1024       # MKWS_DETECT_LIVE_MAX_NEW


def live_history(average_window_duration_ms, hop_samples, sample_rate=16000):
    """The `history` a live detector needs: the most windows an average can span.  Window w is at floor(w * hop_ms) with hop_ms =
    hop_samples * 1000 / sample_rate, so two windows k apart are more than k * hop_ms - 1 ms apart; the host deque keeps those within
    average_window_duration_ms of the newest: k < (avg + 1) / hop_ms, i.e. at most floor((avg + 1) / hop_ms) + 1 windows.  ValueError
    above LIVE_MAX_HISTORY (the C call refuses it too, rather than ever averaging over too few windows)."""
    if not average_window_duration_ms >= 0:
        raise ValueError("average_window_duration_ms must be >= 0")
    if hop_samples <= 0 or sample_rate <= 0 or hop_samples * 1000 < sample_rate:
        raise ValueError("the hop must be at least one millisecond")
    avg = float(average_window_duration_ms)
    history = (int(np.floor((avg + 1) * sample_rate / (hop_samples * 1000))) if np.isfinite(avg) else LIVE_MAX_HISTORY) + 1
    if history > LIVE_MAX_HISTORY:
        raise ValueError(f"an average over {average_window_duration_ms} ms spans {history} windows of {hop_samples} samples; "
                         f"the live detector keeps at most {LIVE_MAX_HISTORY}")
    return history


def live_detector_state(n_heads, n_thr, history, device=None):
    """A zero-filled state block (int64 CUDA tensor) = a fresh stream.  Reset is .zero_(), snapshot .clone(), restore .copy_()."""
    import torch
    n = _lib.lib().mkws_detect_live_state_bytes(int(n_heads), int(n_thr), int(history))
    if n == 0 and n_heads:
        raise ValueError(f"no live detector state for {n_heads} heads x {n_thr} thresholds with a history of {history} "
                         f"(thresholds: 1 .. 1024, history: 1 .. {LIVE_MAX_HISTORY})")
    return torch.zeros(max(1, n // 8), dtype=torch.int64, device=device if device is not None else "cuda")


def live_out_words(n_heads, n_thr, max_new):
    """int64 words of detect_live_step's output buffer: the counts (int32 pairs padded to whole words), then the events."""
    return (n_heads * n_thr + 1) // 2 + 2 * n_heads * n_thr * max_new


def live_unpack(words, n_heads, n_thr, max_new):
    """The host copy (numpy int64) of that buffer -> (counts int32 [N, T], events EVENT_DTYPE [N, T, max_new]; `window` counts inside the push)."""
    cwords = (n_heads * n_thr + 1) // 2
    return (words[:cwords].view(np.int32)[:n_heads * n_thr].reshape(n_heads, n_thr),
            words[cwords:].view(EVENT_DTYPE).reshape(n_heads, n_thr, max_new))


def detect_live_step(state, probs, meta, d_thresholds, average_window_duration_ms, suppression_ms, minimum_count, history, target_id=2,
                     fired_only=False, out=None, scores=None):
    """One step of the live detector.  state: live_detector_state(N, T, history); probs CUDA float32 [N, max_new, C]; meta CUDA int64
    [2 + max_new] = {count, first new window, time_ms of each new window} (what Frontend.live_push writes); d_thresholds CUDA float64
    [T].  -> out, a CUDA int64 tensor of live_out_words(N, T, max_new) words (live_unpack reads its host copy): the events and counts of
    THIS push.  scores: optional CUDA float64 [N, max_new].  Steps whose windows add up to a stream give, concatenated, detect_on_device
    on the whole stream byte for byte.  Asynchronous, allocation-free when `out` is passed in, one launch: capturable."""
    import torch
    if not torch.is_tensor(probs) or not probs.is_cuda:
        raise ValueError("probs must be a contiguous CUDA float32 tensor [heads, max_new, classes]")
    N, max_new, C, T = check_live_step(probs.device, state, probs, meta, d_thresholds, history, out, scores)
    if out is None:
        out = torch.zeros(live_out_words(N, T, max_new), dtype=torch.int64, device=probs.device)
    base = out.data_ptr()
    with torch.cuda.device(probs.device):
        _lib.check(_lib.lib().mkws_detect_live_step(
            state.data_ptr(), probs.data_ptr(), meta.data_ptr(), max_new, N, C, int(target_id), d_thresholds.data_ptr(), T,
            float(average_window_duration_ms), float(suppression_ms), int(minimum_count), int(bool(fired_only)), int(history),
            base + 8 * ((N * T + 1) // 2), base, scores.data_ptr() if scores is not None else None, _lib.current_stream_ptr()))
    return out


def check_live_step(device, state, probs, meta, d_thresholds, history, out=None, scores=None):
    """What detect_live_step refuses, decided before any device call -> (N, max_new, classes, T).  probs contiguous float32 [N, max_new,
    classes]; d_thresholds contiguous float64 of T values; meta contiguous int64 of at least 2 + max_new elements; state a contiguous
    int64 tensor of at least mkws_detect_live_state_bytes(N, T, history) bytes (a size of 0 for N > 0 = arguments the C call refuses in its
    own words, before it looks at a buffer: the state's size is then not judged here); out (if given) contiguous int64 of at least
    live_out_words(N, T, max_new) words; scores (if given) contiguous float64 of at least N * max_new values; all on `device`.
    ValueError otherwise."""
    import torch
    from .frontend import _describe
    if not torch.is_tensor(probs) or probs.dim() != 3 or probs.dtype != torch.float32 or not probs.is_contiguous() or probs.device != device:
        raise ValueError(f"detect_live_step: probs must be a contiguous float32 tensor [heads, max_new, classes] on {device}, got {_describe(probs)}")
    N, max_new, C = (int(v) for v in probs.shape)
    if not torch.is_tensor(d_thresholds) or d_thresholds.dtype != torch.float64 or not d_thresholds.is_contiguous() or \
            d_thresholds.device != device:
        raise ValueError(f"detect_live_step: d_thresholds must be a contiguous float64 tensor [T] on {device}, got {_describe(d_thresholds)}")
    T = int(d_thresholds.numel())
    if not torch.is_tensor(meta) or meta.dtype != torch.int64 or meta.numel() < 2 + max_new or not meta.is_contiguous() or meta.device != device:
        raise ValueError(f"detect_live_step: meta must be a contiguous int64 tensor [2 + max_new = {2 + max_new}] on {device}, got {_describe(meta)}")
    need = _lib.lib().mkws_detect_live_state_bytes(N, T, int(history))
    if not torch.is_tensor(state) or state.dtype != torch.int64 or not state.is_contiguous() or 8 * state.numel() < need or state.device != device:
        raise ValueError(f"detect_live_step: state must be a contiguous int64 tensor of at least {(need + 7) // 8} words on {device} "
                         f"(live_detector_state({N}, {T}, {int(history)})), got {_describe(state)}")
    words = live_out_words(N, T, max_new)
    if out is not None and (not torch.is_tensor(out) or out.dtype != torch.int64 or out.numel() < words or not out.is_contiguous() or out.device != device):
        raise ValueError(f"detect_live_step: out must be a contiguous int64 tensor of {words} words (live_out_words) on {device}, got {_describe(out)}")
    if scores is not None and (not torch.is_tensor(scores) or scores.dtype != torch.float64 or scores.numel() < N * max_new or not scores.is_contiguous()
                               or scores.device != device):
        raise ValueError(f"detect_live_step: scores must be a contiguous float64 tensor [{N}, {max_new}] on {device}, got {_describe(scores)}")
    return N, max_new, C, T


# Many streams in lockstep (mkws_detect_live_step_many): S detectors stepped in one launch.  The host specification is one
# LiveDetectorHost per stream.

def live_detector_state_many(streams, n_heads, n_thr, history, device=None):
    """Zero-filled state blocks of `streams` fresh streams: an int64 CUDA tensor [streams, words]; the row stride is the state stride, so
    row s viewed flat is a valid one-stream state (detect_live_step takes it, .zero_() resets that stream alone)."""
    import torch
    if int(streams) < 0:
        raise ValueError(f"live_detector_state_many: {streams} streams")
    words = live_detector_state(n_heads, n_thr, history, device=device).numel()
    return torch.zeros((int(streams), words), dtype=torch.int64, device=device if device is not None else "cuda")


def live_out_words_many(streams, n_heads, n_thr, max_new):
    """int64 words of detect_live_step_many's output buffer: ALL counts [S, N, T] (int32 pairs padded to whole words), then ALL events
    [S, N, T, max_new]."""
    return (streams * n_heads * n_thr + 1) // 2 + 2 * streams * n_heads * n_thr * max_new


def live_unpack_many(words, streams, n_heads, n_thr, max_new):
    """The host copy (numpy int64) of that buffer -> (counts int32 [S, N, T], events EVENT_DTYPE [S, N, T, max_new]); [s] of each is what
    live_unpack gives for stream s alone."""
    cwords = (streams * n_heads * n_thr + 1) // 2
    return (words[:cwords].view(np.int32)[:streams * n_heads * n_thr].reshape(streams, n_heads, n_thr),
            words[cwords:].view(EVENT_DTYPE).reshape(streams, n_heads, n_thr, max_new))


def detect_live_step_many(states, probs, meta, d_thresholds, average_window_duration_ms, suppression_ms, minimum_count, history, target_id=2,
                          fired_only=False, out=None, scores=None):
    """One step of S live detectors.  states: live_detector_state_many(S, N, T, history); probs CUDA float32 [N, S * max_new, C], stream
    s's windows in rows s * max_new .. of every head's plane (what Head.forward_many gives for the batch Frontend.live_push_many filled);
    meta CUDA int64 [S, 2 + max_new] as live_push_many writes it; d_thresholds CUDA float64 [T].  -> out, a CUDA int64 tensor of
    live_out_words_many(S, N, T, max_new) words (live_unpack_many reads its host copy).  scores: optional CUDA float64 [S, N, max_new].
    For every stream this is detect_live_step on its own slice, byte for byte; a meta row with count == 0 leaves its stream as it is.
    Asynchronous, allocation-free when `out` is passed in, one launch for any S: capturable."""
    import torch
    from .frontend import check_live_many, check_live_many_tensors
    if meta.dim() != 2 or meta.shape[1] < 2:
        raise ValueError("meta must be an int64 tensor [streams, 2 + max_new]")
    max_new = int(meta.shape[1]) - 2
    check_live_many(states, meta.shape, 2 + max_new, "meta")
    S = int(states.shape[0])
    if probs.dim() != 3 or probs.shape[1] != S * max_new:
        raise ValueError(f"probs must have the shape [heads, {S} x {max_new}, classes]: max_new rows per stream in every head's plane")
    if not probs.is_cuda or probs.dtype != torch.float32 or not probs.is_contiguous():
        raise ValueError("probs must be a contiguous CUDA float32 tensor [heads, streams * max_new, classes]")
    N, _, C = probs.shape
    T = int(d_thresholds.numel())
    if d_thresholds.dtype != torch.float64 or not d_thresholds.is_cuda or meta.dtype != torch.int64 or not meta.is_cuda or not meta.is_contiguous():
        raise ValueError("d_thresholds must be CUDA float64 [T] and meta contiguous CUDA int64 [streams, 2 + max_new]")
    words = live_out_words_many(S, N, T, max_new)
    if out is not None and (out.numel() != words or out.dtype != torch.int64 or not out.is_contiguous()):
        raise ValueError(f"out must be a contiguous int64 tensor of {words} words (live_out_words_many)")
    if scores is not None and (scores.numel() != S * N * max_new or scores.dtype != torch.float64 or not scores.is_contiguous()):
        raise ValueError(f"scores must be a contiguous float64 tensor [{S}, {N}, {max_new}]")
    check_live_many_tensors("detect_live_step_many", probs.device, states=(states, torch.int64), meta=(meta, torch.int64),
                            d_thresholds=(d_thresholds, torch.float64), out=(out, torch.int64), scores=(scores, torch.float64))
    if not d_thresholds.is_contiguous():
        raise ValueError("detect_live_step_many: d_thresholds must be contiguous")
    if out is None:                            # (nothing is allocated before everything the caller gave has been accepted)
        out = torch.zeros(words, dtype=torch.int64, device=probs.device)
    base = out.data_ptr()
    with torch.cuda.device(probs.device):
        _lib.check(_lib.lib().mkws_detect_live_step_many(
            states.data_ptr(), 8 * int(states.stride(0)), S, probs.data_ptr(), meta.data_ptr(), max_new, N, C, int(target_id),
            d_thresholds.data_ptr(), T, float(average_window_duration_ms), float(suppression_ms), int(minimum_count), int(bool(fired_only)),
            int(history), base + 8 * ((S * N * T + 1) // 2), base, scores.data_ptr() if scores is not None else None, _lib.current_stream_ptr()))
    return out


# Routes (mkws_detect_live_step_routes): R detectors of one head each, route r listening to slot route_slot[r] with its own threshold row.
# The host specification is one LiveDetectorHost(1, thresholds of the route) per route, fed its slot's pushes.

def live_detector_state_routes(n_routes, n_thr, history, device=None):
    """Zero-filled state blocks of `n_routes` fresh routes: an int64 CUDA tensor [n_routes, words]; row r viewed flat is the one-stream state
    of one head (detect_live_step takes it, .zero_() resets that route alone)."""
    return live_detector_state_many(n_routes, 1, n_thr, history, device=device)


def live_out_words_routes(n_routes, n_thr, max_new):
    """int64 words of detect_live_step_routes' output buffer: the many-stream layout with streams = n_routes, n_heads = 1."""
    return live_out_words_many(n_routes, 1, n_thr, max_new)


def live_unpack_routes(words, n_routes, n_thr, max_new):
    """The host copy (numpy int64) of that buffer -> (counts int32 [R, T], events EVENT_DTYPE [R, T, max_new])."""
    counts, events = live_unpack_many(words, n_routes, 1, n_thr, max_new)
    return counts[:, 0], events[:, 0]


def check_live_routes(states, probs, meta, route_slot, thresholds, out=None, scores=None):
    """What detect_live_step_routes refuses, decided before any device call -> (R, n_slots, max_new, classes, T).  states int64
    [R, words] with contiguous, non-overlapping rows; probs contiguous float32 [R * max_new, classes] (or [R, max_new, classes]); meta
    contiguous int64 [n_slots, 2 + max_new]; route_slot contiguous int32 [R]; thresholds contiguous float64 [R, T]; out contiguous int64
    of live_out_words_routes words; scores contiguous float64 of R * max_new values.  ValueError otherwise."""
    import torch
    from .frontend import check_live_many
    if not torch.is_tensor(meta) or meta.dim() != 2 or meta.shape[1] < 2 or meta.dtype != torch.int64 or not meta.is_contiguous():
        raise ValueError("meta must be a contiguous int64 tensor [slots, 2 + max_new]")
    n_slots, max_new = int(meta.shape[0]), int(meta.shape[1]) - 2
    if not torch.is_tensor(route_slot) or route_slot.dim() != 1 or route_slot.dtype != torch.int32 or not route_slot.is_contiguous():
        raise ValueError("route_slot must be a contiguous int32 vector [routes]")
    check_live_many(states, (int(states.shape[0]) if states.dim() == 2 else 0, 1), 1, "states")      # (the rules of the state tensor itself)
    if int(route_slot.shape[0]) != int(states.shape[0]):
        raise ValueError(f"route_slot has {int(route_slot.shape[0])} entries for the {int(states.shape[0])} rows of the state tensor: one per route")
    R = int(states.shape[0])
    if not torch.is_tensor(thresholds) or thresholds.dim() != 2 or int(thresholds.shape[0]) != R or thresholds.shape[1] < 1 or \
            thresholds.dtype != torch.float64 or not thresholds.is_contiguous():
        raise ValueError(f"thresholds must be a contiguous float64 tensor [{R}, T]: one row per route")
    T = int(thresholds.shape[1])
    if not torch.is_tensor(probs) or probs.dim() not in (2, 3) or probs.dtype != torch.float32 or not probs.is_contiguous() or \
            int(probs.numel()) != R * max_new * int(probs.shape[-1]) or (probs.dim() == 3 and int(probs.shape[0]) != R):
        raise ValueError(f"probs must be a contiguous float32 tensor [{R} x {max_new}, classes]: max_new rows per route")
    C = int(probs.shape[-1])
    words = live_out_words_routes(R, T, max_new)
    if out is not None and (out.numel() != words or out.dtype != torch.int64 or not out.is_contiguous()):
        raise ValueError(f"out must be a contiguous int64 tensor of {words} words (live_out_words_routes)")
    if scores is not None and (scores.numel() != R * max_new or scores.dtype != torch.float64 or not scores.is_contiguous()):
        raise ValueError(f"scores must be a contiguous float64 tensor [{R}, {max_new}]")
    return R, n_slots, max_new, C, T


def detect_live_step_routes(states, probs, meta, route_slot, d_thresholds, average_window_duration_ms, suppression_ms, minimum_count, history,
                            target_id=2, fired_only=False, out=None, scores=None):
    """One step of R routed live detectors.  states: live_detector_state_routes(R, T, history); probs CUDA float32 [R * max_new, C] (or
    [R, max_new, C]), route r's windows in rows r * max_new .. (what HeadGroup.forward_routes writes); meta CUDA int64 [n_slots, 2 +
    max_new] as Frontend.live_push_many writes it; route_slot CUDA int32 [R], the slot whose meta row a route follows (outside
    [0, n_slots): the route is disabled, its state untouched, its counts zero); d_thresholds CUDA float64 [R, T], a row per route.
    -> out, a CUDA int64 tensor of live_out_words_routes(R, T, max_new) words (live_unpack_routes, or live_unpack_many with streams = R
    and n_heads = 1, reads its host copy).  scores: optional CUDA float64 [R, max_new].  For every route this is detect_live_step with one
    head on its own state row, byte for byte.  Asynchronous, allocation-free when `out` is passed in, one launch for any R: capturable."""
    import torch
    R, n_slots, max_new, C, T = check_live_routes(states, probs, meta, route_slot, d_thresholds, out, scores)
    for name, t in (("probs", probs), ("meta", meta), ("route_slot", route_slot), ("d_thresholds", d_thresholds), ("states", states)):
        if not t.is_cuda:
            raise ValueError(f"{name} must be a CUDA tensor")
    for name, t in (("meta", meta), ("route_slot", route_slot), ("d_thresholds", d_thresholds), ("states", states), ("out", out), ("scores", scores)):
        if t is not None and t.device != probs.device:
            raise ValueError(f"{name} must live on the device of probs ({probs.device}), not {t.device}")
    if out is None:
        out = torch.zeros(live_out_words_routes(R, T, max_new), dtype=torch.int64, device=probs.device)
    base = out.data_ptr()
    with torch.cuda.device(probs.device):
        _lib.check(_lib.lib().mkws_detect_live_step_routes(
            states.data_ptr(), 8 * int(states.stride(0)), R, route_slot.data_ptr(), n_slots, probs.data_ptr(), meta.data_ptr(), max_new, C,
            int(target_id), d_thresholds.data_ptr(), T, float(average_window_duration_ms), float(suppression_ms), int(minimum_count),
            int(bool(fired_only)), int(history), base + 8 * ((R * T + 1) // 2), base, scores.data_ptr() if scores is not None else None,
            _lib.current_stream_ptr()))
    return out


class LiveDetectorHost:
    """The host restatement of the live detector: K x T SingleTargetRecognizeCommands (one per keyword head and threshold) fed push by
    push.  step() returns what one mkws_detect_live_step leaves behind, and is the specification it is held to bit for bit."""

    def __init__(self, n_heads, thresholds, average_window_duration_ms, suppression_ms, minimum_count, target_id=2, fired_only=False, classes=3):
        self.n_heads, self.thresholds = int(n_heads), [float(t) for t in thresholds]
        self.settings = (average_window_duration_ms, suppression_ms, minimum_count)
        self.target_id, self.fired_only, self.classes = int(target_id), bool(fired_only), int(classes)
        self.reset()

    def reset(self):
        from .embedding.single_target_recognize_commands import SingleTargetRecognizeCommands
        avg, sup, minc = self.settings
        labels = ["_class_%d" % c for c in range(self.classes)]       # (the class reports "_silence_" for everything but the target)
        labels[self.target_id] = self._keyword = "_keyword_"
        self.lanes = [[SingleTargetRecognizeCommands(labels, avg, thr, sup, minc, self.target_id) for thr in self.thresholds]
                      for _ in range(self.n_heads)]

    def step(self, probs, times_ms):
        """probs [K, n, classes], times_ms [n]: the windows of one push (n may be 0) -> (counts int32 [K, T], events: [K][T] arrays of
        EVENT_DTYPE with `window` counted inside the push, scores float64 [K, n])."""
        from .embedding.single_target_recognize_commands import RecognizeResult
        probs = np.asarray(probs)
        K, T, n = self.n_heads, len(self.thresholds), len(times_ms)
        counts, scores = np.zeros((K, T), np.int32), np.zeros((K, n), np.float64)
        events = [[[] for _ in range(T)] for _ in range(K)]
        el = RecognizeResult()
        for k in range(K):
            for j in range(T):
                rc = self.lanes[k][j]
                for i in range(n):
                    rc.process_latest_result(probs[k, i], int(times_ms[i]), el)
                    scores[k, i] = el.score
                    fired = el.is_new_command and el.found_command == self._keyword
                    if el.is_new_command and (fired or not self.fired_only):
                        events[k][j].append((i, int(fired), el.score))
                counts[k, j] = len(events[k][j])
        return counts, [[np.asarray(e, dtype=EVENT_DTYPE) for e in row] for row in events], scores

