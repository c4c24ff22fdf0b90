"""Shared by the live-session tests: the scripted stream of probabilities and the host reference it is held to."""
import numpy as np

from multilingual_kws_amd.embedding.single_target_recognize_commands import RecognizeResult, SingleTargetRecognizeCommands

THRESHOLDS = [0.3, 0.5, 0.7, 0.9]
SETTINGS = [(100, 500, 4), (40, 60, 2), (0, 0, 1), (300, 1000, 4)]      # (average_window_duration_ms, suppression_ms, minimum_count)
WINDOWS, HOP_MS = 240, 20
SHIFTS = (0, 13, 27)


def scripted_probs(shifts=SHIFTS):
    """float32 [len(shifts), 240, 3]: 40 quiet windows, 40 loud ones, ... with a little noise; head k is the pattern shifted by shifts[k]."""
    w = np.arange(WINDOWS)
    conf = (np.where((w // 40) % 2, 0.93, 0.05) + 0.04 * np.random.default_rng(0).random(WINDOWS)).astype(np.float32)
    planes = [np.roll(conf, s) for s in shifts]
    return np.stack([np.stack([1 - c, np.zeros_like(c), c], axis=1) for c in planes]).astype(np.float32)


def times_ms(n=WINDOWS):
    return [HOP_MS * i for i in range(n)]


def lane_reference(probs_head, times, thr, avg, sup, minc):
    """One SingleTargetRecognizeCommands fed window by window -> [(window, fired, score)] of its is_new_command steps."""
    rc, el, out = SingleTargetRecognizeCommands(["_silence_", "_unknown_", "kw"], avg, thr, sup, minc, 2), RecognizeResult(), []
    for w, t in enumerate(times):
        rc.process_latest_result(probs_head[w], t, el)
        if el.is_new_command:
            out.append((w, int(el.found_command == "kw"), el.score))
    return out


def push_plan(n_windows, h, leading_empty=0):
    """[(first window, count)]: `leading_empty` empty pushes, then pushes of h windows with a ragged last one."""
    return [(0, 0)] * leading_empty + [(s, min(h, n_windows - s)) for s in range(0, n_windows, h)]
