"""Device streaming detector: host wrapper over mkws_detect_stream (include/mkws.h).

SingleTargetRecognizeCommands (embedding/single_target_recognize_commands.py) stepped over every window of a stream, for N keyword
heads x T detection thresholds in one launch.  The host class is the specification: labels, is_new_command and the float64 scores
are equal bit for bit (tests/test_detector_device.py).  score_on_device goes on to mkws_detect_score: the fires of every lane matched
against ground-truth times on the device, embedding/tpr_fpr.py being the specification (tests/test_operating_curve_gpu.py)."""
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


def detect_on_device(probs, times_ms, thresholds, average_window_duration_ms, suppression_ms, minimum_count, target_id=2, trace=False,
                     fired_only=False):
    """probs: CUDA tensor [N, W, C], float32 or float64 (made contiguous if it is a view), or a numpy array, which is uploaded.
    times_ms: W non-decreasing integers.  thresholds: T floats.  -> DetectResult; never a cut event list.  One launch and one
    device-to-host copy (= one synchronisation) per call; a second round only if a lane had more events than event_capacity() allows
    for (fired_only=False on a stream with quiet stretches)."""
    import torch
    times = check_times(times_ms)                                      # before anything touches the device
    thr = np.ascontiguousarray(np.asarray(thresholds, dtype=np.float64).reshape(-1))
    if thr.size < 1:
        raise ValueError("at least one threshold")
    if not average_window_duration_ms >= 0:
        raise ValueError("average_window_duration_ms must be >= 0")
    if not torch.is_tensor(probs):
        a = np.asarray(probs)
        probs = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64 if a.dtype == np.float64 else np.float32)).cuda()
    if probs.dim() != 3 or not probs.is_cuda or probs.dtype not in (torch.float32, torch.float64):
        raise ValueError("probs must be a CUDA tensor or numpy array [heads, windows, classes] of float32 or float64")
    N, W, C = probs.shape
    if W != times.shape[0]:
        raise ValueError(f"{W} windows but {times.shape[0]} timestamps")
    if not 0 <= int(target_id) < C:
        raise ValueError(f"target_id {target_id} outside [0, {C})")
    probs = probs.contiguous()
    T = int(thr.size)
    if N == 0 or W == 0:                                               # nothing to launch (the C call would write nothing either)
        return DetectResult(np.zeros((N, T), np.int32), np.zeros((N, T, 0), EVENT_DTYPE),
                            np.zeros((N, W), np.float64) if trace else None, np.zeros((N, T, W), np.uint8) if trace else None)
    L = _lib.lib()
    dev = probs.device
    with torch.cuda.device(dev):
        # times and thresholds travel in one upload: int64 times, then the float64 thresholds' bit patterns
        host_in = np.concatenate([times, thr.view(np.int64)])
        d_in = torch.from_numpy(host_in).to(dev, non_blocking=True)
        d_scores = torch.empty((N, W), dtype=torch.float64, device=dev) if trace else None
        d_flags = torch.empty((N, T, W), dtype=torch.uint8, device=dev) if trace else None
        cap = event_capacity(times, suppression_ms, fired_only)
        while True:
            # counts (int32 pairs padded to whole 8-byte words) and events in ONE buffer, so that they cross in one copy
            cwords = (N * T + 1) // 2
            d_out = torch.empty(cwords + 2 * N * T * cap, dtype=torch.int64, device=dev)
            base = d_out.data_ptr()
            _lib.check(L.mkws_detect_stream(
                probs.data_ptr(), int(probs.dtype == torch.float64), N, W, C, int(target_id), d_in.data_ptr(), d_in.data_ptr() + 8 * W, T,
                float(average_window_duration_ms), float(suppression_ms), int(minimum_count), int(bool(fired_only)),
                base + 8 * cwords, cap, base, d_scores.data_ptr() if trace else None, d_flags.data_ptr() if trace else None,
                _lib.current_stream_ptr()))
            out = d_out.cpu().numpy()                                  # the call's one synchronisation
            counts = out[:cwords].view(np.int32)[:N * T].reshape(N, T)
            if counts.size == 0 or int(counts.max()) <= cap:
                break
            cap = W                                                    # a lane cannot have more events than windows
        events = out[cwords:].view(EVENT_DTYPE).reshape(N, T, cap)
        return DetectResult(counts, events, d_scores.cpu().numpy() if trace else None, d_flags.cpu().numpy() if trace else None)


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
    One upload (times, thresholds, ground truth, offsets), two launches, one copy of 16 * N * T bytes: no event list reaches the host."""
    import torch
    times = check_times(times_ms)
    thr = np.ascontiguousarray(np.asarray(thresholds, dtype=np.float64).reshape(-1))
    if thr.size < 1:
        raise ValueError("at least one threshold")
    if not average_window_duration_ms >= 0:
        raise ValueError("average_window_duration_ms must be >= 0")
    tol = float(time_tolerance_ms)
    if not tol >= 0:
        raise ValueError("time_tolerance_ms must be >= 0")
    # the device forms t +- tol in float64; CPython does so too for a float tolerance and exactly for an int one: the same while both fit 2^53
    span = max(abs(int(times[0])), abs(int(times[-1]))) if times.size else 0
    if span > 2 ** 53 or (np.isfinite(tol) and span + tol > 2 ** 53):
        raise ValueError("times_ms (and times_ms +- time_tolerance_ms) must lie within +-2**53 milliseconds: they are compared as float64")
    gt, offsets = pack_groundtruth(gt_times_per_head, len(probs))       # refused before anything is uploaded
    if not torch.is_tensor(probs):
        a = np.asarray(probs)
        probs = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64 if a.dtype == np.float64 else np.float32)).cuda()
    if probs.dim() != 3 or not probs.is_cuda or probs.dtype not in (torch.float32, torch.float64):
        raise ValueError("probs must be a CUDA tensor or numpy array [heads, windows, classes] of float32 or float64")
    N, W, C = probs.shape
    if W != times.shape[0]:
        raise ValueError(f"{W} windows but {times.shape[0]} timestamps")
    if not 0 <= int(target_id) < C:
        raise ValueError(f"target_id {target_id} outside [0, {C})")
    T = int(thr.size)
    if N == 0:
        return np.zeros((0, T, 3), np.int32)
    probs = probs.contiguous()
    L = _lib.lib()
    dev = probs.device
    with torch.cuda.device(dev):
        # one upload of 8-byte words: int64 times, the bit patterns of the float64 thresholds and ground truth, the int32 offsets in pairs
        off_words = np.zeros((N + 2) // 2 * 2, np.int32)
        off_words[:N + 1] = offsets
        host_in = np.concatenate([times, thr.view(np.int64), gt.view(np.int64), off_words.view(np.int64)])
        d_in = torch.from_numpy(host_in).to(dev, non_blocking=True)
        p_times = d_in.data_ptr()
        p_thr, p_gt, p_off = p_times + 8 * W, p_times + 8 * (W + T), p_times + 8 * (W + T + gt.size)
        cap = event_capacity(times, suppression_ms, fired_only=True)
        d_events = torch.empty(2 * N * T * cap, dtype=torch.int64, device=dev)
        d_counts = torch.empty(N * T, dtype=torch.int32, device=dev)
        d_tally = torch.empty((N, T, 4), dtype=torch.int32, device=dev)
        stream = _lib.current_stream_ptr()
        _lib.check(L.mkws_detect_stream(
            probs.data_ptr(), int(probs.dtype == torch.float64), N, W, C, int(target_id), p_times, p_thr, T,
            float(average_window_duration_ms), float(suppression_ms), int(minimum_count), 1, d_events.data_ptr(), cap, d_counts.data_ptr(),
            None, None, stream))
        _lib.check(L.mkws_detect_score(d_events.data_ptr(), d_counts.data_ptr(), N, T, cap, p_times, W, p_gt, p_off, tol, d_tally.data_ptr(), stream))
        tally = d_tally.cpu().numpy()                                  # the call's one synchronisation: 16 bytes per lane
    if tally[:, :, 3].any():
        n, k = (int(x[0]) for x in np.nonzero(tally[:, :, 3]))
        raise RuntimeError(f"head {n}, threshold {k}: {int(tally[n, k, 0])} fires for an event list of {cap}; the list was cut and cannot be scored")
    return np.ascontiguousarray(tally[:, :, :3])


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


def _segment_probs(probs, rows):
    import torch
    if not torch.is_tensor(probs):
        a = np.asarray(probs)
        probs = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64 if a.dtype == np.float64 else np.float32)).cuda()
    if probs.dim() != 2 or not probs.is_cuda or probs.dtype not in (torch.float32, torch.float64):
        raise ValueError("probs must be a CUDA tensor or numpy array [rows, classes] of float32 or float64")
    if probs.shape[0] != rows:
        raise ValueError(f"{probs.shape[0]} rows of probabilities but {rows} timestamps")
    return probs.contiguous()


def _segment_capacity(times, off, suppression_ms, fired_only):
    """The largest event_capacity over the segments, and the longest segment."""
    spans = list(zip(off[:-1].tolist(), off[1:].tolist()))
    return (max([event_capacity(times[a:b], suppression_ms, fired_only) for a, b in spans], default=0),
            max([b - a for a, b in spans], default=0))


def detect_segments_on_device(probs, seg_offsets, times_ms, thresholds, average_window_duration_ms, suppression_ms, minimum_count, target_id=2,
                              trace=False, fired_only=False):
    """detect_on_device for S concatenated recordings: probs CUDA tensor (or numpy array, which is uploaded) [rows, C], float32 or
    float64; segment s = rows seg_offsets[s] .. seg_offsets[s + 1] with its own non-decreasing times_ms[those rows]; thresholds: T
    floats.  -> SegmentDetectResult whose segment s equals detect_on_device on that slice alone; never a cut event list.  One upload,
    one launch and one device-to-host copy per call; a second round at the longest segment's length only if a lane had more events
    than the largest event_capacity() over the segments allows for."""
    import torch
    off, times = check_segments(seg_offsets, times_ms)                 # before anything touches the device
    thr = np.ascontiguousarray(np.asarray(thresholds, dtype=np.float64).reshape(-1))
    if thr.size < 1:
        raise ValueError("at least one threshold")
    if not average_window_duration_ms >= 0:
        raise ValueError("average_window_duration_ms must be >= 0")
    R, S, T = int(times.shape[0]), int(off.shape[0]) - 1, int(thr.size)
    probs = _segment_probs(probs, R)
    C = probs.shape[1]
    if not 0 <= int(target_id) < C:
        raise ValueError(f"target_id {target_id} outside [0, {C})")
    spans = list(zip(off[:-1].tolist(), off[1:].tolist()))
    if S == 0:
        return SegmentDetectResult(np.zeros((0, T), np.int32), np.zeros((0, T, 0), EVENT_DTYPE), [] if trace else None, [] if trace else None)
    L = _lib.lib()
    dev = probs.device
    with torch.cuda.device(dev):
        # times, thresholds and offsets travel in one upload of 8-byte words
        off_words = np.zeros((S + 2) // 2 * 2, np.int32)
        off_words[:S + 1] = off
        d_in = torch.from_numpy(np.concatenate([times, thr.view(np.int64), off_words.view(np.int64)])).to(dev, non_blocking=True)
        p_times = d_in.data_ptr()
        p_thr, p_off = p_times + 8 * R, p_times + 8 * (R + T)
        d_scores = torch.empty(R, dtype=torch.float64, device=dev) if trace else None
        d_flags = torch.empty(T * R, dtype=torch.uint8, device=dev) if trace else None
        cap, longest = _segment_capacity(times, off, suppression_ms, fired_only)
        while True:
            cwords = (S * T + 1) // 2
            d_out = torch.empty(cwords + 2 * S * T * cap, dtype=torch.int64, device=dev)
            base = d_out.data_ptr()
            _lib.check(L.mkws_detect_segments(
                probs.data_ptr(), int(probs.dtype == torch.float64), p_off, S, R, C, int(target_id), p_times, p_thr, T,
                float(average_window_duration_ms), float(suppression_ms), int(minimum_count), int(bool(fired_only)),
                base + 8 * cwords, cap, base, d_scores.data_ptr() if trace else None, d_flags.data_ptr() if trace else None,
                _lib.current_stream_ptr()))
            out = d_out.cpu().numpy()                                  # the call's one synchronisation
            counts = out[:cwords].view(np.int32)[:S * T].reshape(S, T)
            if int(counts.max()) <= cap:
                break
            cap = longest                                              # a lane cannot have more events than its segment has windows
        events = out[cwords:].view(EVENT_DTYPE).reshape(S, T, cap)
        scores = flags = None
        if trace:
            h_scores, h_flags = d_scores.cpu().numpy(), d_flags.cpu().numpy()
            scores = [h_scores[a:b] for a, b in spans]
            flags = [h_flags[T * a:T * b].reshape(T, b - a) for a, b in spans]
        return SegmentDetectResult(counts, events, scores, flags)


def score_segments_on_device(probs, seg_offsets, times_ms, thresholds, gt_times_per_segment, time_tolerance_ms, average_window_duration_ms,
                             suppression_ms, minimum_count, target_id=2):
    """score_on_device for S concatenated recordings (mkws_detect_segments + mkws_detect_score_segments): -> int32 [S, T, 3] = (found,
    true_positives_raw, false_negatives) per (segment, threshold) lane; segment s equals score_on_device on that slice with
    gt_times_per_segment[s].  One upload, two launches, one copy of 16 * S * T bytes; RuntimeError if a lane's event list was cut."""
    import torch
    off, times = check_segments(seg_offsets, times_ms)
    thr = np.ascontiguousarray(np.asarray(thresholds, dtype=np.float64).reshape(-1))
    if thr.size < 1:
        raise ValueError("at least one threshold")
    if not average_window_duration_ms >= 0:
        raise ValueError("average_window_duration_ms must be >= 0")
    tol = float(time_tolerance_ms)
    if not tol >= 0:
        raise ValueError("time_tolerance_ms must be >= 0")
    span = int(np.abs(times).max()) if times.size else 0
    if span > 2 ** 53 or (np.isfinite(tol) and span + tol > 2 ** 53):
        raise ValueError("times_ms (and times_ms +- time_tolerance_ms) must lie within +-2**53 milliseconds: they are compared as float64")
    R, S, T = int(times.shape[0]), int(off.shape[0]) - 1, int(thr.size)
    gt, gt_off = pack_groundtruth(gt_times_per_segment, S)             # refused before anything is uploaded
    probs = _segment_probs(probs, R)
    C = probs.shape[1]
    if not 0 <= int(target_id) < C:
        raise ValueError(f"target_id {target_id} outside [0, {C})")
    if S == 0:
        return np.zeros((0, T, 3), np.int32)
    L = _lib.lib()
    dev = probs.device
    with torch.cuda.device(dev):
        words = np.zeros((2, (S + 2) // 2 * 2), np.int32)
        words[0, :S + 1], words[1, :S + 1] = off, gt_off
        host_in = np.concatenate([times, thr.view(np.int64), gt.view(np.int64), words[0].view(np.int64), words[1].view(np.int64)])
        d_in = torch.from_numpy(host_in).to(dev, non_blocking=True)
        p_times = d_in.data_ptr()
        p_thr, p_gt = p_times + 8 * R, p_times + 8 * (R + T)
        p_off = p_gt + 8 * gt.size
        p_gt_off = p_off + 4 * words.shape[1]
        cap, _ = _segment_capacity(times, off, suppression_ms, True)
        d_events = torch.empty(2 * S * T * cap, dtype=torch.int64, device=dev)
        d_counts = torch.empty(S * T, dtype=torch.int32, device=dev)
        d_tally = torch.empty((S, T, 4), dtype=torch.int32, device=dev)
        stream = _lib.current_stream_ptr()
        _lib.check(L.mkws_detect_segments(
            probs.data_ptr(), int(probs.dtype == torch.float64), p_off, S, R, C, int(target_id), p_times, p_thr, T,
            float(average_window_duration_ms), float(suppression_ms), int(minimum_count), 1, d_events.data_ptr(), cap, d_counts.data_ptr(),
            None, None, stream))
        _lib.check(L.mkws_detect_score_segments(d_events.data_ptr(), d_counts.data_ptr(), p_off, S, R, T, cap, p_times, p_gt, p_gt_off, tol,
                                                d_tally.data_ptr(), stream))
        tally = d_tally.cpu().numpy()                                  # the call's one synchronisation: 16 bytes per lane
    if tally[:, :, 3].any():
        s, k = (int(x[0]) for x in np.nonzero(tally[:, :, 3]))
        raise RuntimeError(f"segment {s}, threshold {k}: {int(tally[s, k, 0])} fires for an event list of {cap}; the list was cut and cannot be scored")
    return np.ascontiguousarray(tally[:, :, :3])
