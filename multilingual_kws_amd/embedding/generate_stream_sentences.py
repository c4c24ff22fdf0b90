"""Drop-in for multilingual_kws/embedding/generate_stream_sentences.py on MI355X: the streaming tests' recordings and their labels.

The reference strings target and non-target sentences into one long WAV with one sox process per piece and one for the join, and
writes the label file from the pieces' durations (generate_stream_and_labels, :144-245; the same recipe with `keyword,time_ms` rows in
luganda/luganda.py:164-217).  Here the pieces are float32 audio in device memory: compose_streams lays R streams out, fades, scales
and sums their pieces, puts them over a looped background bed at a given gain or a given signal-to-noise ratio and clips, all R streams
in one mkws_stream_mix launch (compose.py); write_streams adds one mkws_pcm_encode launch and the files;
generate_stream_and_labels keeps the reference's file names and label formats.  MP3 input, TextGrid and Common Voice bookkeeping stay
out, as in word_extraction.py."""
import math
import os
from dataclasses import dataclass
from typing import Any, Optional

import numpy as np

from .. import compose
from . import input_data


@dataclass
class StreamPiece:
    """One piece of a stream.  audio: a WAV path, a CUDA tensor or an array, mono at the stream's rate (a file at another rate is
    converted); start_s / end_s: the word inside a target piece, in seconds of the piece; gain: a factor on every sample; fade_ms: a
    linear fade-in and fade-out; gap_ms: silence after the piece; overlap_ms: how far the next piece starts before this one ends (a
    cross-fade when both fade)."""
    audio: Any
    is_target: bool = False
    keyword: Optional[str] = None
    start_s: Optional[float] = None
    end_s: Optional[float] = None
    gain: float = 1.0
    fade_ms: float = 0.0
    gap_ms: float = 0.0
    overlap_ms: float = 0.0


def ms_to_frames(ms, rate):
    """floor(ms * rate / 1000 + 0.5): the frames of a gap, an overlap or a fade."""
    return int(math.floor(float(ms) * int(rate) / 1000 + 0.5))


def plan_stream(lengths, pieces, rate):
    """Host only: the frames of every piece and the pieces -> (out_start of every piece, n_out), exact integers.  A piece starts where
    the one before it ended, plus that piece's gap, minus its overlap; the stream ends with its last sample or its last gap, whichever
    is later."""
    starts, at, n_out = [], 0, 0
    for n, p in zip(lengths, pieces):
        n, gap, overlap = int(n), ms_to_frames(p.gap_ms, rate), ms_to_frames(p.overlap_ms, rate)
        if gap < 0 or overlap < 0 or overlap > n:
            raise ValueError(f"plan_stream: gap_ms = {p.gap_ms}, overlap_ms = {p.overlap_ms} on a piece of {n} frames")
        starts.append(at)
        n_out = max(n_out, at + n)
        at += n + gap - overlap
        n_out = max(n_out, at)
    return starts, n_out


def stream_labels(pieces, lengths, rate, target_word=None):
    """([(keyword, start_ms)], target_times_s) of one stream as the reference computes them (:222-244): a running float
    `current += frames / rate` per piece -- what sox reports as a wav's duration -- and for a target piece
    (current + float(start_s), current + float(end_s)), start_ms = start * 1000.  A gap or an overlap moves `current` by its own
    frames / rate after the piece.  keyword: the piece's own, else target_word."""
    labels, times = [], []
    current = 0
    for p, n in zip(pieces, lengths):
        if p.is_target:
            start = current + float(p.start_s)
            times.append((start, current + float(p.end_s)))
            labels.append((p.keyword if p.keyword is not None else target_word, start * 1000))
        current += int(n) / rate
        shift = ms_to_frames(p.gap_ms, rate) - ms_to_frames(p.overlap_ms, rate)
        if shift:
            current += shift / rate
    return labels, times


def _is_path(a):
    return isinstance(a, (str, os.PathLike))


def _per_stream(value, R, what):
    """A scalar or one value per stream -> a list of R."""
    if value is None:
        return None
    if isinstance(value, (list, tuple, np.ndarray)) and not np.isscalar(value) and np.ndim(value) == 1:
        if len(value) != R:
            raise ValueError(f"compose_streams: {len(value)} values of {what} for {R} streams")
        return list(value)
    return [value] * R


class _Sources:
    """Every distinct source (a piece's audio, a bed) once in one flat float32 buffer, each at a multiple of four floats."""

    def __init__(self, on_device, rate, dev):
        self.on_device, self.rate, self.dev = on_device, rate, dev
        self.parts, self.seen, self.total = [], {}, 0

    def add(self, audio):
        """-> (offset, length) of the source in the flat buffer."""
        import torch
        key = os.fspath(audio) if _is_path(audio) else id(audio)
        if key in self.seen:
            return self.seen[key][:2]
        if _is_path(audio):
            if self.on_device:
                a = input_data.read_recording(audio, self.rate, device=self.dev)
            else:
                with open(audio, "rb") as fh:
                    a, file_rate = input_data.decode_wav(fh.read(), -1)
                if file_rate != self.rate:
                    raise ValueError(f"{os.fspath(audio)}: a file at {file_rate} Hz needs the device to be converted to {self.rate} Hz")
        elif torch.is_tensor(audio) and audio.is_cuda:
            if not self.on_device:
                raise ValueError("compose_streams: a CUDA tensor with device='cpu'")
            a = audio.to(torch.float32).reshape(-1)
        else:
            a = input_data._host_audio(audio).reshape(-1)
        n = int(a.shape[0])
        self.seen[key] = (self.total, n, audio)                 # the object is kept, so that its id stays its own
        self.parts.append(a)
        at, self.total = self.total, (self.total + n + 3) & ~3
        return at, n

    def flat(self):
        import torch
        if not self.on_device:
            out = np.zeros(max(self.total, 4), np.float32)
            for a, (at, n, _) in zip(self.parts, self.seen.values()):
                out[at:at + n] = a
            return out
        # host parts travel in one upload; everything is joined by one concatenation
        host = [i for i, a in enumerate(self.parts) if not torch.is_tensor(a) or not a.is_cuda]
        if host:
            sizes = [int(self.parts[i].shape[0]) for i in host]
            up = torch.from_numpy(np.concatenate([np.asarray(self.parts[i], np.float32) for i in host] + [np.zeros(1, np.float32)]))
            up = up.to(self.dev, non_blocking=True)
            for i, a in zip(host, torch.split(up[:-1], sizes)):
                self.parts[i] = a
        pad = torch.zeros(4, dtype=torch.float32, device=self.dev)
        pieces = []
        for a in self.parts:
            pieces.append(a.to(self.dev))
            pieces.append(pad[:(-int(a.shape[0])) & 3])
        pieces.append(pad)
        return torch.cat(pieces)


def _use_device(streams, background, device):
    import torch
    if device is not None:
        return torch.device(device).type != "cpu"
    every = [p.audio for pieces in streams for p in pieces]
    if background is not None:
        every += list(background) if isinstance(background, (list, tuple)) else [background]
    if any(torch.is_tensor(a) and a.is_cuda for a in every):
        return True
    return torch.cuda.is_available()


@dataclass
class Composed:
    """What compose_streams makes, with the plan behind it."""
    audio: Any
    lengths: list
    offsets: list
    labels: list
    bed_gain: Any
    target_times_s: list
    piece_lengths: list
    items: Any = None
    descs: Any = None
    src: Any = None


def _compose(streams, rate=16000, background=None, snr_db=None, bed_gain=None, bed_start=0, clip=True, device=None):
    import torch
    streams = [list(pieces) for pieces in streams]
    R, rate = len(streams), int(rate)
    if background is None and (snr_db is not None or bed_gain is not None):
        raise ValueError("compose_streams: snr_db and bed_gain need a background")
    if background is not None and (snr_db is None) == (bed_gain is None):
        raise ValueError("compose_streams: a background needs exactly one of snr_db and bed_gain")
    on_device = _use_device(streams, background, device)
    dev = input_data._cuda_device(device) if on_device else None
    sources = _Sources(on_device, rate, dev)
    beds = None
    if background is not None:
        beds = list(background) if isinstance(background, (list, tuple)) else [background] * R
        if len(beds) != R:
            raise ValueError(f"compose_streams: {len(beds)} backgrounds for {R} streams")
    starts_of_bed = _per_stream(bed_start, R, "bed_start")

    item_rows, desc_rows, labels, times, lengths, offsets, piece_lengths, at_out = [], [], [], [], [], [], [], 0
    for r, pieces in enumerate(streams):
        spans = [sources.add(p.audio) for p in pieces]
        ns = [n for _, n in spans]
        starts, n_out = plan_stream(ns, pieces, rate)
        for p, (so, n), at in zip(pieces, spans, starts):
            fade = ms_to_frames(p.fade_ms, rate)
            if fade < 0:
                raise ValueError(f"compose_streams: fade_ms = {p.fade_ms}")
            item_rows.append((so, n, 0, n, at, fade, fade, float(p.gain), r))
        bo, bl, bs = 0, 0, 0
        if beds is not None:
            bo, bl = sources.add(beds[r])
            if bl == 0:
                raise ValueError(f"compose_streams: the background of stream {r} is empty")
            bs = int(starts_of_bed[r]) % bl
        desc_rows.append((at_out, n_out, bo, bl, bs))
        lab, tm = stream_labels(pieces, ns, rate)
        labels.append(lab)
        times.append(tm)
        lengths.append(n_out)
        offsets.append(at_out)
        piece_lengths.append(ns)
        at_out += n_out
    items = compose.make_stream_items(item_rows)
    descs = compose.make_stream_descs(desc_rows, items)
    src = sources.flat()
    total = max(at_out, 1)

    if not on_device:
        gains = None
        if beds is not None:
            if bed_gain is not None:
                gains = np.asarray(_per_stream(bed_gain, R, "bed_gain"), dtype=np.float32)
            else:
                p_fg, p_bed = compose.power_host(src, items, descs)
                gains = compose.bed_gain_host(p_fg, p_bed, descs, compose.snr_scale(_per_stream(snr_db, R, "snr_db")))
        audio = compose.mix_host(src, items, descs, gains, clip, out_floats=total)[:at_out]
        return Composed(audio, lengths, offsets, labels, gains, times, piece_lengths, items, descs, src)

    with torch.cuda.device(dev):
        compose.check_stream_tables(items, descs, int(src.numel()), total, max(lengths, default=0))
        tables = compose.upload_tables(items, descs, dev)
        gains = None
        if beds is not None:
            if bed_gain is not None:
                if torch.is_tensor(bed_gain) and bed_gain.is_cuda:
                    gains = bed_gain.to(torch.float32).reshape(-1).contiguous()
                    if gains.numel() != R:
                        raise ValueError(f"compose_streams: {gains.numel()} values of bed_gain for {R} streams")
                else:
                    g = bed_gain.tolist() if torch.is_tensor(bed_gain) else bed_gain
                    gains = torch.from_numpy(np.asarray(_per_stream(g, R, "bed_gain"), dtype=np.float32)).to(dev, non_blocking=True)
            else:
                scale = compose.snr_scale(_per_stream(snr_db, R, "snr_db"))
                partials, bad_p = compose.power_on_device(src, items, descs, validate=False, check=False, tables=tables)
                gains = compose.bed_gain_on_device(partials, descs, scale, tables=tables)
        out = torch.empty(total, dtype=torch.float32, device=dev)
        out, bad = compose.mix_on_device(src, items, descs, gains, clip, out=out, validate=False, check=False, tables=tables)
        n_bad = int(bad.cpu()[0])
    if n_bad:
        raise ValueError(f"mkws_stream_mix refused {n_bad} of {len(items)} items and {R} streams")
    return Composed(out[:at_out], lengths, offsets, labels, gains, times, piece_lengths, items, descs, src)


def compose_streams(streams, rate=16000, background=None, snr_db=None, bed_gain=None, bed_start=0, clip=True, device=None):
    """streams: a list of lists of StreamPiece -> (audio, lengths, offsets, labels, bed_gain): the R streams one after another in one
    float32 buffer [sum of lengths] (stream r is audio[offsets[r]:offsets[r] + lengths[r]]), the [(keyword, start_ms)] labels of every
    stream (stream_labels) and the gain every bed was given (None without a background).

    background: a path, a tensor or an array looped under the whole stream from its sample bed_start on, or one per stream; exactly
    one of bed_gain (the factor on it) and snr_db (the factor is found from the stream's own foreground and bed power, so that
    10 log10 of their ratio after the factor is snr_db) goes with it, a scalar or one per stream.  clip: the result is limited to
    [-1, 1].  Paths are read by input_data.read_recording at `rate`; every distinct source goes once into one flat buffer.

    On a device (a CUDA piece, a GPU in the machine, or `device`): ONE mkws_stream_mix launch for all R streams, preceded with snr_db
    by mkws_stream_power and mkws_stream_bed_gain with no host round trip in between.  Without a GPU (or with device="cpu") host arrays
    go through compose.mix_host and give the same audio bits for the same gains."""
    c = _compose(streams, rate, background, snr_db, bed_gain, bed_start, clip, device)
    return c.audio, c.lengths, c.offsets, c.labels, c.bed_gain


def _stream_images(c, rate, format):
    return input_data._encode_images(c.audio, [[(o, n, 0, n, 0, 0, 1.0)] for o, n in zip(c.offsets, c.lengths)], int(rate), format)


def write_streams(streams, paths=None, rate=16000, format="s16", **compose_kw):
    """compose_streams, then every stream encoded as a mono WAV file in `format` (pcm.FORMATS) by ONE mkws_pcm_encode launch and one
    download (input_data.encode_wav's core, fed the streams' lengths) -> (the paths written, or the file images when paths is None,
    labels, bed_gain)."""
    c = _compose(streams, rate, **compose_kw)
    images = _stream_images(c, rate, format)
    return (images if paths is None else input_data._write_images(images, paths)), c.labels, c.bed_gain


def label_lines(labels, target_word=None, label_style="sentences"):
    """The label file's lines: "sentences" is the reference's f"{target_word}, {start_ms}" (:241-244), "csv" luganda's
    f"{keyword},{time_ms}" (luganda/luganda.py:208-217).  Both are read back by batch_streaming_analysis._read_groundtruth."""
    if label_style not in ("sentences", "csv"):
        raise ValueError(f'label_style must be "sentences" or "csv", not {label_style!r}')
    lines = []
    for kw, t_ms in labels:
        kw = target_word if kw is None or (label_style == "sentences" and target_word is not None) else kw
        lines.append(f"{kw}, {t_ms}\n" if label_style == "sentences" else f"{kw},{t_ms}\n")
    return lines


def generate_stream_and_labels(dest_dir, wav_data, target_word, clips_dir=None, rate=16000, format="s16", label_style="sentences",
                               **compose_kw):
    """The reference's generate_stream_and_labels (:144-245) without its sox processes: wav_data is its list of dicts -- is_target,
    start_s, end_s, and `wav` (a path, or the audio itself) or `mp3name_no_ext` (resolved as clips_dir/<name>.wav); the optional keys
    keyword, gain, fade_ms, gap_ms and overlap_ms are StreamPiece's.  Writes dest_dir/streaming_test.wav (mono, `format`, at `rate`) and
    dest_dir/streaming_labels.txt and asserts, as the reference does, that neither exists -> target_times_s, its list of
    (start_s, end_s) of every target word in the stream."""
    dest_dir = os.fspath(dest_dir)
    assert os.path.isdir(dest_dir), "no dest dir available"
    label_file, wav_stream_file = os.path.join(dest_dir, "streaming_labels.txt"), os.path.join(dest_dir, "streaming_test.wav")
    assert not os.path.isfile(label_file), "label file exists already"
    assert not os.path.isfile(wav_stream_file), "wav stream exists already"
    pieces = []
    for comp in wav_data:
        audio = comp.get("wav")
        if audio is None:
            assert clips_dir is not None and os.path.isdir(clips_dir), "clips data not found"
            audio = os.path.join(os.fspath(clips_dir), comp["mp3name_no_ext"] + ".wav")
        if _is_path(audio) and not os.path.exists(audio):
            raise ValueError("could not find", audio)
        extra = {k: comp[k] for k in ("keyword", "gain", "fade_ms", "gap_ms", "overlap_ms") if k in comp}
        pieces.append(StreamPiece(audio, bool(comp["is_target"]), start_s=comp.get("start_s"), end_s=comp.get("end_s"), **extra))
    c = _compose([pieces], rate, **compose_kw)
    input_data._write_images(_stream_images(c, rate, format), [wav_stream_file])
    with open(label_file, "w") as fh:
        fh.writelines(label_lines(c.labels[0], target_word, label_style))
    return c.target_times_s[0]
