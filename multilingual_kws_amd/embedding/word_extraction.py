"""Drop-in for the audio side of multilingual_kws/embedding/word_extraction.py (reference :175-231): a word cut out of a long recording by
its forced-alignment times into a one-second training shot, on the device.

The reference runs one sox process per shot: convert to 16 kHz, `trim`, `fade` 25 ms in and out, then `pad` to one second.  Here the
recording is already model-rate float32 audio in device memory (input_data.read_recording), and all the shots of a recording leave in
ONE mkws_pcm_encode launch (include/mkws.h, "Device audio encoded into WAV sample data") and one download.

sox applies `fade` before `pad`, so the fades lie on the word's own frames and not on the padding.  An encode item fades at its own
first and last frames, so a padded shot is written as up to THREE encode items whose byte ranges abut in the file's sample data: the
front padding, the word with its fades, the back padding.  A padding item reads in front of the recording (start = -n_frames), where
every frame is +0.0f by the item's own rule: no zero buffer exists.  A shot that needs no padding is one item.

The MP3 side of extract_shot_from_mp3 is not here (there is no MP3 decoder in this build), nor the TextGrid and Common Voice
bookkeeping of the reference module, which is plain Python and runs unchanged."""
import math
import os

import numpy as np

from . import input_data


def extract_one_second(duration_s: float, start_s: float, end_s: float):
    """One second around the midpoint between start_s and end_s, kept inside [0, duration_s] (reference :175-190) -> (start_s, end_s).
    A recording shorter than a second is returned whole."""
    if duration_s < 1:
        return (0, duration_s)
    center_s = start_s + ((end_s - start_s) / 2.0)
    new_start_s = center_s - 0.5
    new_end_s = center_s + 0.5
    if new_end_s > duration_s:
        new_end_s = duration_s
        new_start_s = duration_s - 1.0
    if new_start_s < 0:
        new_start_s = 0
        new_end_s = np.minimum(duration_s, new_start_s + 1.0)
    return (new_start_s, new_end_s)


def _frame(t_s, rate):
    return int(math.floor(t_s * rate + 0.5))


def shot_items(rate, n_samples, timings, include_context=False, fade_s=0.025):
    """The geometry of extract_shot_from_mp3 (reference :207-231) in frames of a recording of n_samples samples at `rate`: for every
    (start_s, end_s) of `timings` the list of the shot's pieces (start, n_frames, fade_in, fade_out), which follow one another in the
    shot.  The pieces' frames add up to exactly `rate` wherever the reference gives about one second (a recording shorter than a second
    gives its own length, as extract_one_second does).
      end_s - start_s < 1 and not include_context: the word's own span [s0, s1), s0 = floor(start_s * rate + 0.5) and s1 likewise, with
        (rate - (s1 - s0)) // 2 zero frames in front of it and the rest behind: [front padding], the word, [back padding];
      otherwise: the extract_one_second window, `rate` frames from floor(window start * rate + 0.5), one piece, no padding.
    The fades (fade_s seconds each, floor(fade_s * rate + 0.5) frames) lie on the word's piece only, as sox applies `fade` before `pad`.
    They are LINEAR: i / fade_in and (n - 1 - i) / fade_out.  sox's default fade curve is not reproduced: it cannot be compared
    against here, where sox does not exist."""
    rate, n_samples = int(rate), int(n_samples)
    fade = max(0, _frame(fade_s, rate))
    shots = []
    for start_s, end_s in timings:
        if end_s - start_s < 1 and not include_context:
            s0, s1 = _frame(start_s, rate), _frame(end_s, rate)
            n = min(max(s1 - s0, 0), rate)
            front = (rate - n) // 2
            back = rate - n - front
            pieces = [(-front, front, 0, 0), (s0, n, fade, fade), (-back, back, 0, 0)]
            shots.append([p for k, p in enumerate(pieces) if k == 1 or p[1] > 0])
        else:
            w0, _ = extract_one_second(n_samples / rate, start_s, end_s)
            n = rate if n_samples >= rate else n_samples
            shots.append([(min(_frame(w0, rate), n_samples - n), n, fade, fade)])
    return shots


def extract_shots(recording, timings, dests=None, rate=16000, include_context=False, format="s16", fade_s=0.025):
    """extract_shot_from_mp3 for every (start_s, end_s) of `timings` over ONE recording: a float32 CUDA tensor [samples] at `rate` (what
    input_data.read_recording returns), a numpy array (encoded on the host, byte for byte the same), or the path of a WAV file of any
    supported format, read and brought to `rate` on the device.  All shots leave in one mkws_pcm_encode launch -> the WAV file images
    (bytes), or, with dests (one path per timing), the paths written."""
    if isinstance(recording, (str, os.PathLike, bytes, bytearray, memoryview)):
        recording = input_data.read_recording(recording, rate)
    host = input_data._host_audio(recording)
    audio = recording.reshape(-1) if host is None else host.reshape(-1)
    n = int(audio.shape[0])
    images = [[(0, n, st, nf, fi, fo, 1.0) for st, nf, fi, fo in pieces] for pieces in shot_items(rate, n, timings, include_context, fade_s)]
    files = input_data._encode_images(audio if host is not None or audio.is_contiguous() else audio.contiguous(), images, rate, format)
    return files if dests is None else input_data._write_images(files, dests)
