"""Drop-in for the streaming-inference core of multilingual_kws/embedding/batch_streaming_analysis.py.

The reference (:99-117) slices a long recording into 1 s windows every 20 ms, calls the micro-frontend op
on each window in a Python loop and runs one full model per keyword.  Here one call produces every
window's features on the GPU with per-frame FFT / filterbank work shared across the 49x-overlapping
windows (mkws_frontend_stream_f32; bit-identical to per-window calls), the embedding is computed once and
any number of few-shot heads are applied to it.  The detector runs on the device as well: detect_many steps
every keyword head and every detection threshold over the stream in one launch (mkws_detect_stream, ..detector);
SingleTargetRecognizeCommands and detect() are its host restatement -- the yardstick the device path is held to bit
for bit, and the path for hosts without a GPU.  StreamTarget / eval_stream_test (:188-241) are the per-keyword entry points run.py drives; multi_keyword_detections is
their multi-keyword form on ONE shared embedding pass (run.py:89-152 runs one full model per keyword).  operating_curves /
multi_keyword_operating_curves go on from the detector to tpr_fpr's summary per keyword and threshold without leaving the device
(mkws_detect_score); tpr_fpr.tpr_fpr is their yardstick and their path on a host without a GPU."""
import math
import os
import pickle
from dataclasses import dataclass
from typing import List, Optional

import numpy as np

from . import input_data
from ..streams import concurrent_streams
from .single_target_recognize_commands import RecognizeResult, SingleTargetRecognizeCommands


@dataclass(frozen=True)
class StreamFlags:
    wav: os.PathLike
    ground_truth: os.PathLike
    target_keyword: str
    detection_thresholds: List[float]
    clip_duration_ms: int = 1000
    clip_stride_ms: int = 20
    average_window_duration_ms: int = 100
    suppression_ms: int = 500
    time_tolerance_ms: int = 750
    minimum_count: int = 4
    max_chunk_length_sec: int = 1200

    def labels(self) -> List[str]:
        return [input_data.SILENCE_LABEL, input_data.UNKNOWN_WORD_LABEL, self.target_keyword]


def window_offsets(data_samples, clip_duration_samples, clip_stride_samples):
    """Start sample of every window the reference evaluates: range(0, data_samples - clip, stride)."""
    return list(range(0, data_samples - clip_duration_samples, clip_stride_samples))


def chunk_audio(audio, max_chunk_samples):
    """The reference's chunking of a long recording (:72-86), AS SHIPPED: recordings shorter than max_chunk_samples are
    one chunk; otherwise, for offset in range(0, n, max_chunk_samples), a chunk that would run past the end is cut to
    [offset, offset + max) and every OTHER chunk is the whole remainder audio[offset:] (the condition is inverted in the
    reference, so all chunks but the last overlap everything after them).  Each chunk is windowed on its own and the
    inferences are concatenated, which is what callers of the reference get back."""
    n = audio.shape[0]
    if max_chunk_samples is None or n < max_chunk_samples:
        return [audio]
    chunks = []
    for offset in range(0, n, int(max_chunk_samples)):
        if offset + max_chunk_samples > n:
            chunks.append(audio[offset:offset + int(max_chunk_samples)])
        else:
            chunks.append(audio[offset:])
    return chunks


def stream_spectrograms(model_settings, audio, clip_duration_samples, clip_stride_samples):
    """float32 audio [n] -> CUDA tensor [num_windows, frames, channels], windows as window_offsets()."""
    import torch
    audio_t = torch.as_tensor(np.asarray(audio, dtype=np.float32)) if not torch.is_tensor(audio) else audio
    audio_t = audio_t.cuda().contiguous()
    n = audio_t.shape[0]
    nwin = len(window_offsets(n, clip_duration_samples, clip_stride_samples))
    frames, chans = model_settings["spectrogram_length"], model_settings["fingerprint_width"]
    if nwin <= 0:
        return torch.empty((0, frames, chans), dtype=torch.float32, device=audio_t.device)
    if model_settings.get("preprocess", "micro") != "micro":      # mfcc / average: the same dispatch as input_data.to_features
        fe = input_data._spectral_for(model_settings, n)
    else:
        fe = input_data._frontend_for(model_settings, n)
    if clip_stride_samples % model_settings["window_stride_samples"] != 0:
        # hop not a multiple of the frame step: no frame sharing possible, fall back to explicit windows
        idx = (torch.arange(clip_duration_samples, device=audio_t.device)[None]
               + torch.arange(nwin, device=audio_t.device)[:, None] * clip_stride_samples)
        return fe.forward(audio_t[idx])
    return fe.stream(audio_t, clip_duration_samples, clip_stride_samples)[:nwin]


class _BatchGraph:
    """embedding.forward + every head over `lanes` FULL batches of `batch` spectrograms, one captured hipGraph PER LANE, each replayed on its
    own HIP stream (static inputs / outputs); cached per (embedding handle, head handles, batch, lanes).

    Why lanes: at 256 windows every launch of the embedding is latency-bound -- one clip per workgroup, each workgroup streaming the whole
    block's weights -- and a 256-clip batch costs about half of what a 1024-clip batch costs.  The batches of a stream are independent: `lanes`
    of them run side by side, every lane on a replica handle (= its own workspace; the heads are read-only and shared) that runs the PLAN of
    lanes x batch clips (4-clip workgroups, 8-clip pairs: a quarter of the chip per launch at four lanes; EmbeddingModel.serving_lanes).
    Round 6: the lanes used to be the branches of ONE forked hipGraph, which this HIP runtime replays one branch after the other (649 k clips/s
    at 4 x 256 where four graphs on four streams give 1.03 M; profiles/r06_notes.md section 8).  One lane = the caller's own handle and plan,
    the same launches as an eager call, bit for bit."""
    _cache = {}

    def __init__(self, embedding, heads, batch, lanes=1):
        import torch
        dev = embedding.device
        ems = embedding.serving_lanes(lanes, max(lanes, SERVING_LANES) * batch) if lanes > 1 else [embedding]
        self.keep = (ems, list(heads))                               # the graphs hold raw handles: keep their owners alive
        self.owner = embedding
        self.lanes = lanes
        self.heals = 0                                               # re-captures after a failed exchange (run)
        self.generation = (embedding.generation, tuple(h.generation for h in heads))
        self.specs = [torch.zeros((batch, 49, 40), dtype=torch.float32, device=dev) for _ in range(lanes)]
        # one stream per lane, each on a hardware queue of its own (measured, not assumed: streams.py); a single lane runs on the caller's stream
        self.side = concurrent_streams(lanes, dev) if lanes > 1 else [None]
        assert len(self.side) == lanes, "serve_spectrograms asks for no more lanes than concurrent_streams() finds"
        self._capture()

    def _capture(self):
        import torch
        from ..head import Head
        ems, heads = self.keep
        lanes, dev, side = self.lanes, ems[0].device, self.side

        def chain(i):
            return Head.forward_many(heads, ems[i].forward(self.specs[i]))
        warm = [torch.cuda.Stream(device=dev)] if lanes == 1 else side
        for i in range(lanes):                                       # eager warm-up on side streams (lazy init outside the capture); a
            warm[i].wait_stream(torch.cuda.current_stream(dev))      # handle with a recorded exchange failure is healed here (the wrapper
            with torch.cuda.stream(warm[i]):                         # repeats the call that returns MKWS_ERR_EXCHANGE)
                chain(i)
            torch.cuda.current_stream(dev).wait_stream(warm[i])
        self.graphs, self.probs = [], []
        for i in range(lanes):
            g = torch.cuda.CUDAGraph()
            if lanes == 1:
                with torch.cuda.graph(g):
                    self.probs.append(chain(i))
            else:
                with torch.cuda.graph(g, stream=side[i]):
                    self.probs.append(chain(i))
            self.graphs.append(g)

    @classmethod
    def get(cls, embedding, heads, batch, lanes=1):
        # keyed on the handles AND their generation counters: a handle closed and re-created at the same address must not hit a graph
        # that still points into the freed one
        key = (id(embedding), embedding.h.value, tuple(h.h.value for h in heads), int(batch), int(lanes))
        gen = (embedding.generation, tuple(h.generation for h in heads))
        g = cls._cache.get(key)
        if g is not None and g.generation != gen:
            g = None
        if g is None:
            if len(cls._cache) >= 8:
                cls._cache.clear()
            g = cls._cache[key] = cls(embedding, heads, batch, lanes)
        return g

    @classmethod
    def forget(cls, obj):
        """Drop every cached graph that captured `obj` (an EmbeddingModel or Head being closed)."""
        for k in [k for k, g in cls._cache.items() if obj is g.owner or any(obj is e for e in g.keep[0]) or any(obj is h for h in g.keep[1])]:
            del cls._cache[k]

    def exchange_failed(self):
        return any(e.get_option("exchange_error") for e in self.keep[0])

    def run(self, parts):
        """parts: `lanes` tensors [batch,49,40] -> list of [n_heads, batch, 3] (views of the static outputs).  Asynchronous: the results are
        ordered behind the caller's current stream, like any other launch on it."""
        import torch
        if self.exchange_failed():
            # an earlier replay ran a failed pair / cluster exchange (its results were NaN): the captured launches would poison every
            # later batch too.  Heal the handles (eager pass) and capture again -- the new graphs hold the single-workgroup kernels
            self._capture()
            self.heals += 1
        if self.lanes == 1:
            self.specs[0].copy_(parts[0])
            self.graphs[0].replay()
            return self.probs
        main = torch.cuda.current_stream(self.owner.device)
        for i in range(self.lanes):                                  # fork: lane i starts where the caller's stream is now (its input is ready there) ...
            self.side[i].wait_stream(main)
            with torch.cuda.stream(self.side[i]):
                self.specs[i].copy_(parts[i])
                self.graphs[i].replay()
        for i in range(self.lanes):                                  # ... and the caller's stream continues behind every lane
            main.wait_stream(self.side[i])
        return self.probs

    def run_all(self, specs, nfull, tail=None):
        """The first `nfull` FULL batches of specs [windows, 49, 40] -> [n_heads, nfull * batch, 3] on the caller's stream.  Batch j runs on lane
        j % lanes; a lane works through its batches back to back on its own stream (copy in, replay, copy out) and the caller's stream joins the
        lanes ONCE, after `tail()` (the eager pass over a ragged last batch, which so runs beside the lanes).  A join after every round of
        `lanes` batches costs a third of the throughput: the lanes drift apart and every round then waits for its slowest (0.99 -> 1.34 ms per
        4 x 256 clips, profiles/r06_notes.md section 8)."""
        import torch
        if self.exchange_failed():
            self._capture()
            self.heals += 1
        bw = self.specs[0].shape[0]
        dev = self.owner.device
        out = torch.empty((len(self.keep[1]), nfull * bw, 3), dtype=torch.float32, device=dev)       # the caller's stream owns the result
        main = torch.cuda.current_stream(dev)
        if self.lanes == 1:
            for j in range(nfull):
                self.specs[0].copy_(specs[j * bw:(j + 1) * bw])
                self.graphs[0].replay()
                out[:, j * bw:(j + 1) * bw].copy_(self.probs[0])
            return out, (tail() if tail is not None else None)
        for i in range(min(self.lanes, nfull)):
            self.side[i].wait_stream(main)
        for j in range(nfull):                                        # issued round-robin so that every lane has work queued early
            i = j % self.lanes
            with torch.cuda.stream(self.side[i]):
                self.specs[i].copy_(specs[j * bw:(j + 1) * bw])
                self.graphs[i].replay()
                out[:, j * bw:(j + 1) * bw].copy_(self.probs[i])
        t = tail() if tail is not None else None
        for i in range(min(self.lanes, nfull)):
            main.wait_stream(self.side[i])
        return out, t


SERVING_LANES = 4      # batches in flight side by side in serve_spectrograms / streaming_inferences (at most: see lane_budget)


def lane_budget(batch, device=None):
    """How many lanes of `batch` clips may run side by side.  The paired kernels of the 2x2-image blocks hold their CU while they wait for their
    partner workgroup (include/mkws.h, failure contract): all lanes' pairs TOGETHER must fit the chip -- 2 workgroups per 8 clips -- or halves
    of different lanes can fill the CUs their partners are waiting for (six lanes of 256 clips: 384 such workgroups for 256 CUs measured 23 ms
    per 2950 windows instead of 3.7, every wait running into the kernels' timeout; profiles/r06_notes.md section 8)."""
    import torch
    cus = torch.cuda.get_device_properties(device if device is not None else torch.cuda.current_device()).multi_processor_count
    return max(1, cus // (2 * ((int(batch) + 7) // 8)))


def serve_spectrograms(emb_model, heads, specs, batch_windows=4096, use_graph=True, graphs_used=None):
    """CUDA spectrograms [windows, 49, 40] -> CUDA softmax outputs [n_heads, windows, 3]: the embedding in batches of
    min(batch_windows, max_batch) windows, every head on every batch.  Asynchronous on the caller's current stream (no host copy, no
    synchronisation): what streaming_inferences runs per chunk and what `bench.py --config stream` times."""
    import torch
    from ..head import Head
    bw = min(batch_windows, emb_model.max_batch)
    nwin = specs.shape[0]
    nfull = nwin // bw if (use_graph and tuple(specs.shape[1:]) == (49, 40)) else 0

    def eager_from(s0):                                       # launch by launch on the caller's own handle: [N, windows, 3] per batch
        return [Head.forward_many(heads, emb_model.forward(specs[s:s + bw])) for s in range(s0, nwin, bw)]
    if nfull == 0:
        parts = eager_from(0)
        return torch.cat(parts, dim=1) if parts else torch.zeros((len(heads), 0, 3), dtype=torch.float32, device=emb_model.device)
    # full batches replay captured graphs, up to SERVING_LANES of them side by side (see _BatchGraph); one lane = the same launches on
    # the same plan as the eager path, bit for bit; several lanes = the workgroup shapes of the clips they hold together
    # (the cluster kernel of small handles spins on up to 14 co-resident members per launch: concurrent lanes could starve
    # each other of CUs, include/mkws.h -- such handles replay one batch at a time)
    lanes = 1 if emb_model.get_option("fuse_cluster") else min(SERVING_LANES, nfull, lane_budget(bw, emb_model.device))
    if lanes > 1:
        lanes = len(concurrent_streams(lanes, emb_model.device))     # (fewer when the runtime has fewer hardware queues to give)
    bg = _BatchGraph.get(emb_model, heads, bw, lanes)
    if graphs_used is not None:
        graphs_used.setdefault(bg, bg.heals)
    full, rest = bg.run_all(specs, nfull, (lambda: eager_from(nfull * bw)) if nfull * bw < nwin else None)
    return torch.cat([full] + list(rest), dim=1) if rest else full


def streaming_inferences(models, model_settings, audio, sample_rate=16000, clip_duration_ms=1000, clip_stride_ms=20,
                         batch_windows=4096, max_chunk_length_sec=None, use_graph=True, _retry=True, as_device=False):
    """Softmax outputs for every window.  `models`: one TransferLearnedModel or a list sharing one embedding
    (multi-keyword serving: the EfficientNet forward runs once, each keyword adds only its 18.5 k-parameter
    head).  Returns [num_windows, 3] (or a list of them) as numpy arrays; with as_device=True the CUDA tensor
    [num_windows, 3] (or [n_models, num_windows, 3] for a list) instead, for detect_many -- after the same
    exchange-failure check and repeat."""
    import torch
    single = not isinstance(models, (list, tuple))
    mlist = [models] if single else list(models)
    clip = int(clip_duration_ms * sample_rate / 1000)
    stride = int(clip_stride_ms * sample_rate / 1000)
    chunks = []                                # per chunk: CUDA [n_models, windows of the chunk, 3]
    emb_model = mlist[0].embedding
    graphs_used = {}                           # graph -> its heal count when this stream first used it

    def degraded():                            # times the handles of this stream have left the exchange kernels after a failure
        return sum(e.get_option("pair_degraded") for e in [emb_model] + list(getattr(emb_model, "_replicas", [])))
    degraded0 = degraded()
    from ..head import Head
    audio_arr = audio if torch.is_tensor(audio) else np.asarray(audio, dtype=np.float32)
    max_chunk = None if max_chunk_length_sec is None else int(max_chunk_length_sec * sample_rate)
    for chunk in chunk_audio(audio_arr, max_chunk):
        specs = stream_spectrograms(model_settings, chunk, clip, stride)
        heads = [m.head for m in mlist]
        chunks.append(serve_spectrograms(emb_model, heads, specs, batch_windows, use_graph, graphs_used))
    if graphs_used:
        # a failed exchange inside a replay leaves NaN rows and no return code: look at the handles once everything has run, and redo
        # the stream on the healed handles (the first run() of the repeat re-captures; a healed handle cannot fail again).  A heal in
        # the middle of the stream -- by a re-capture or by the eager call of a ragged tail -- means earlier batches were poisoned.
        torch.cuda.synchronize(emb_model.device)
        if degraded() != degraded0 or any(g.exchange_failed() or g.heals != h0 for g, h0 in graphs_used.items()):
            if not _retry:
                # the repeat ran with every handle of the stream off the exchange kernels (below): nothing left that could fail this way
                from .._lib import MKWS_ERR_EXCHANGE, MkwsError
                raise MkwsError(MKWS_ERR_EXCHANGE, "an in-kernel exchange failed again while the stream was being repeated on the single-workgroup kernels")
            import warnings
            warnings.warn("multilingual_kws_amd: an in-kernel exchange failed during a graph replay; repeating the stream on the single-workgroup kernels. "
                          "This embedding handle and its serving replicas STAY on that plan for the rest of the process (the library retires a handle's "
                          "exchange kernels for good once one exchange has failed: include/mkws.h, MKWS_ERR_EXCHANGE); create a new handle to get them back",
                          RuntimeWarning)
            # EVERY serving-lane replica leaves the exchange kernels before the repeat, not only the handle whose error word was set: a
            # replica that fails during the repeat would return its NaN rows with nobody looking
            for e in [emb_model] + list(getattr(emb_model, "_replicas", [])):
                if e.get_option("exchange_error"):                              # heals: the wrapper repeats the call that reports the error.  A known
                    e.forward(torch.zeros((1, 49, 40), dtype=torch.float32, device=emb_model.device))   # one-window batch, not the last chunk's (maybe empty) one
                e.set_option("fuse_pair", 0)
                e.set_option("fuse_cluster", 0)
            _BatchGraph.forget(emb_model)                                       # graphs captured on the old plan
            return streaming_inferences(models, model_settings, audio, sample_rate, clip_duration_ms, clip_stride_ms, batch_windows, max_chunk_length_sec,
                                        use_graph, _retry=False, as_device=as_device)
    if as_device:
        if not chunks:
            full = torch.zeros((len(mlist), 0, 3), dtype=torch.float32, device=emb_model.device)
        else:
            full = chunks[0] if len(chunks) == 1 else torch.cat(chunks, dim=1)
        return full[0] if single else full
    res = [torch.cat([c[k] for c in chunks]).cpu().numpy() if chunks else np.zeros((0, 3), np.float32) for k in range(len(mlist))]
    return res[0] if single else res


# Live serving -- StreamingSession, LiveSession and the groups, one window or one push at a time -- is live.py; its names stay importable here
from .live import (LiveGroupScheduler, LivePushCutter, LiveRoutedGroup, LiveRouteTable, LiveSession, LiveSessionGroup,  # noqa: E402,F401
                   StreamingSession, default_live_flags)


def detect(inferences, flags: StreamFlags, threshold, sample_rate=16000, data_samples=None):
    """Runs the detector over per-window softmax outputs; returns (found_words, found_words_w_confidences)
    exactly as the reference collects them (:143-167)."""
    clip = int(flags.clip_duration_ms * sample_rate / 1000)
    stride = int(flags.clip_stride_ms * sample_rate / 1000)
    offsets = window_offsets(data_samples, clip, stride) if data_samples is not None else [i * stride for i in range(len(inferences))]
    element = RecognizeResult()
    rc = SingleTargetRecognizeCommands(labels=flags.labels(), average_window_duration_ms=flags.average_window_duration_ms,
                                       detection_threshold=threshold, suppression_ms=flags.suppression_ms,
                                       minimum_count=flags.minimum_count, target_id=2)
    found, found_conf = [], []
    for ix, off in enumerate(offsets):
        t_ms = int(off * 1000 / sample_rate)
        rc.process_latest_result(inferences[ix], t_ms, element)
        if element.is_new_command and element.found_command != "_silence_":
            found.append([element.found_command, t_ms])
            found_conf.append([element.found_command, t_ms, element.score])
    return found, found_conf


def detection_windows(times_ms, n_samples, sample_rate, before_ms=1000, after_ms=1000, pad=False):
    """[(start, n_frames)] in frames of a recording of n_samples samples: the window [t - before_ms, t + after_ms] of every t of
    times_ms, its ends at floor(ms * sample_rate / 1000).  pad=False: clamped to the recording, as sox `trim` clamps at its end (and
    cannot start in front of it); pad=True: the full window, to be zero-filled where it leaves the recording."""
    windows = []
    for t in times_ms:
        a = math.floor((t - before_ms) * sample_rate / 1000)
        b = max(a, math.floor((t + after_ms) * sample_rate / 1000))
        if not pad:
            a, b = min(max(a, 0), n_samples), min(max(b, 0), n_samples)
        windows.append((a, b - a))
    return windows


def extract_detections(detections, wav, dest_dir=None, target_word=None, before_ms=1000, after_ms=1000, sample_rate=None, format="s16",
                       pad=False):
    """The harvest of luganda/luganda.ipynb cell 21 (one sox `trim` process per detection there): every detection's
    [t - before_ms, t + after_ms] of the recording as a mono WAV file in `format`, all of them cut and encoded in ONE mkws_pcm_encode
    launch and one download (input_data._encode_images).  detections: the [(keyword, time_ms), ...] list detect / eval_stream_test
    return per threshold.  wav: the path of a WAV file of any supported format, read by input_data.read_recording at its own rate
    unless sample_rate is given; or the recording itself with sample_rate, a float32 CUDA tensor [samples] (a numpy array is encoded on
    the host, byte for byte the same).  Windows: detection_windows.  -> with dest_dir (made if absent) the paths written,
    f"{ix:03d}_{target_word}_detection_{time_ms}ms.wav" as in the notebook (target_word defaults to each detection's own keyword);
    without it the file images (bytes)."""
    from .. import pcm
    detections = list(detections)
    if isinstance(wav, (str, os.PathLike, bytes, bytearray, memoryview)):
        image = input_data._wav_image(wav)
        if sample_rate is None:
            sample_rate = pcm.wav_info(image).rate
        wav = input_data.read_recording(image, sample_rate)
    elif sample_rate is None:
        raise ValueError("extract_detections: a recording that is not a file needs its sample_rate")
    host = input_data._host_audio(wav)
    audio = wav.reshape(-1) if host is None else host.reshape(-1)
    if host is None and not audio.is_contiguous():
        audio = audio.contiguous()
    n, rate = int(audio.shape[0]), int(sample_rate)
    windows = detection_windows([t for _, t in detections], n, rate, before_ms, after_ms, pad)
    images = input_data._encode_images(audio, [[(0, n, a, nf, 0, 0, 1.0)] for a, nf in windows], rate, format)
    if dest_dir is None:
        return images
    paths = [os.path.join(os.fspath(dest_dir), f"{ix:03d}_{kw if target_word is None else target_word}_detection_{t}ms.wav")
             for ix, (kw, t) in enumerate(detections)]
    os.makedirs(os.fspath(dest_dir), exist_ok=True)
    return input_data._write_images(images, paths)


def _keyword_planes(inferences, flags, keywords):
    """What detect_many and operating_curves accept as inferences -> (one array or tensor [N, W, classes], whether it is a tensor,
    whether the caller gave [W, classes], the N keywords)."""
    import torch
    as_list = isinstance(inferences, (list, tuple))
    on_device = torch.is_tensor(inferences[0] if as_list and len(inferences) else inferences)
    if as_list:
        inferences = (torch.stack(list(inferences)) if on_device else np.stack([np.asarray(x) for x in inferences])) if len(inferences) \
            else np.zeros((0, 0, 3), np.float32)
    elif not on_device:
        inferences = np.asarray(inferences)
    single = not as_list and inferences.ndim == 2
    if single:
        inferences = inferences[None]
    if inferences.ndim != 3:
        raise ValueError("inferences must be [windows, classes] or [keywords, windows, classes]")
    N = inferences.shape[0]
    keywords = [flags.target_keyword] * N if keywords is None else list(keywords)
    if len(keywords) != N:
        raise ValueError(f"{len(keywords)} keywords for {N} rows of inferences")
    return inferences, on_device, single, keywords


def _stream_windows(inferences, flags, sample_rate, data_samples):
    """-> (clip and stride in samples, the start sample of every window detect() would step over); IndexError, as there, for fewer
    rows of inferences [N, W, classes] than windows."""
    clip = int(flags.clip_duration_ms * sample_rate / 1000)
    stride = int(flags.clip_stride_ms * sample_rate / 1000)
    offsets = window_offsets(data_samples, clip, stride) if data_samples is not None else [i * stride for i in range(inferences.shape[1])]
    if inferences.shape[1] < len(offsets):
        raise IndexError(f"index {inferences.shape[1]} is out of bounds: {inferences.shape[1]} rows of inferences for {len(offsets)} windows")
    return clip, stride, offsets


def _found_by_threshold(keyword, t_ms, thresholds, events, counts):
    """The fired-only events [T, capacity] and their counts [T] of one detector plane, t_ms being the times of its windows
    -> {threshold: (found_words, found_words_w_confidences)}, the lists detect() builds."""
    found = {}
    for k, thr in enumerate(thresholds):
        ev = events[k, :counts[k]]
        when = [t_ms[w] for w in ev["window"].tolist()]
        found[thr] = ([[keyword, t] for t in when], [[keyword, t, s] for t, s in zip(when, ev["score"].tolist())])
    return found


def detect_many(inferences, flags: StreamFlags, thresholds, sample_rate=16000, data_samples=None, keywords=None):
    """detect() for every keyword and every threshold of a stream at once.  inferences: [W, 3] for one keyword, or [N, W, 3] / a list
    of N [W, 3] for several (numpy arrays or CUDA tensors); keywords: the N target words (default: flags.target_keyword for each).
    -> {threshold: (found_words, found_words_w_confidences)} for [W, 3] input, a list of N such dicts otherwise, holding exactly the
    lists detect() builds.  CUDA tensors, and numpy input on a host with a GPU, take ONE device launch for all keywords and thresholds
    (..detector.detect_on_device); numpy input on a host without a GPU loops over detect().  More inference rows than window offsets
    are cut to the offsets (chunk_audio as shipped can return more); fewer raise IndexError, as detect() does."""
    import dataclasses
    import torch
    thresholds = list(thresholds)
    inferences, on_device, single, keywords = _keyword_planes(inferences, flags, keywords)
    N = inferences.shape[0]
    offsets = _stream_windows(inferences, flags, sample_rate, data_samples)[2]
    if not on_device and not torch.cuda.is_available():
        out = [{thr: detect(inferences[n], dataclasses.replace(flags, target_keyword=keywords[n]), thr, sample_rate, data_samples)
                for thr in thresholds} for n in range(N)]
        return out[0] if single else out
    if len(flags.labels()) != inferences.shape[2]:
        raise ValueError("The results for recognition should contain {} elements, but there are {} produced".format(
            len(flags.labels()), inferences.shape[2]))
    from ..detector import detect_on_device
    t_ms = [int(off * 1000 / sample_rate) for off in offsets]
    out = [{} for _ in range(N)]
    if thresholds:
        res = detect_on_device(inferences[:, :len(offsets)], t_ms, thresholds, flags.average_window_duration_ms, flags.suppression_ms,
                               flags.minimum_count, target_id=2, fired_only=True)
        counts = res.counts.tolist()
        out = [_found_by_threshold(keywords[n], t_ms, thresholds, res.event_buffer[n], counts[n]) for n in range(N)]
    return out[0] if single else out


def _groundtruth_times(groundtruth, keywords):
    """Per keyword its ground-truth times in the caller's order: from rows (keyword, time_ms) as run.py reads its CSV, or a dict."""
    if isinstance(groundtruth, dict):
        return [list(groundtruth.get(kw, [])) for kw in keywords]
    rows = list(groundtruth)
    return [[t for k, t in rows if k == kw] for kw in keywords]


def summary_from_tally(keyword, thresh, found, true_positives_raw, false_negatives, n_gt, duration_s, num_nontarget_words=None):
    """tpr_fpr.tpr_fpr's summary dict from the three integers of a (keyword, threshold) lane (..detector.score_on_device), in tpr_fpr's own
    expressions.  -> (dict, whether the true-positive count was capped to n_gt, where tpr_fpr prints its warning)."""
    true_positives = true_positives_raw
    capped = true_positives > n_gt
    if capped:
        true_positives = n_gt
    false_positives = found - true_positives
    result = dict(
        keyword=keyword,
        tpr=true_positives / n_gt,
        thresh=thresh,
        true_positives=true_positives,
        false_positives=false_positives,
        false_negatives=false_negatives,
        false_rejections_per_instance=false_negatives / n_gt,
        false_accepts_per_hour=false_positives / duration_s * 3600,
        groundtruth_positives=n_gt,
    )
    if num_nontarget_words is not None:
        result["fpr"] = false_positives / num_nontarget_words
    return result, capped


def _curve_from_tally(keyword, thresholds, tally, n_gt, duration_s, num_nontarget_words):
    """The tally [T][3] of one scored plane -> (summary_from_tally's dict per threshold, how many of them had their count capped)."""
    curve, capped = [], 0
    for thr, lane in zip(thresholds, tally):
        result, was_capped = summary_from_tally(keyword, thr, *lane, n_gt, duration_s, num_nontarget_words)
        capped += was_capped
        curve.append(result)
    return curve, capped


def _read_groundtruth(path):
    """run.py's ground-truth file: rows `keyword,time_ms`."""
    import csv
    with open(path, "r") as fh:
        return [(row[0], float(row[1])) for row in csv.reader(fh) if row]


def operating_curves(inferences, flags: StreamFlags, thresholds, groundtruth, keywords=None, sample_rate=16000, data_samples=None,
                     duration_s=None, num_nontarget_words=None):
    """The operating curve of every keyword of a stream: tpr_fpr.tpr_fpr's summary dict (true-positive rate, false accepts per hour, ...)
    at every threshold, for detect_many's detections matched against `groundtruth` within flags.time_tolerance_ms.

    inferences, thresholds, keywords, sample_rate, data_samples as detect_many.  groundtruth: rows (keyword, time_ms) as run.py reads
    them from its CSV, or a dict keyword -> times; each keyword's times are used in the order given (tpr_fpr expects them ascending and
    stops its scan early on a list that is not).  duration_s: default data_samples / sample_rate, and without data_samples the samples
    the windows cover, ((windows - 1) * stride + clip) / sample_rate.
    -> for [W, 3] input a list over thresholds of the dicts tpr_fpr(keyword, threshold, detect(...)[0], times, duration_s,
    flags.time_tolerance_ms, num_nontarget_words) returns, equal to them key for key, int for int and float for float; a list of N such
    lists otherwise.  A keyword without ground truth raises ZeroDivisionError, as tpr_fpr does.  tpr_fpr's "WARNING: weird timing issue"
    (more matched detections than occurrences; the count is capped) is printed once per call with the number of lanes it applied to.
    CUDA tensors, and numpy input on a host with a GPU, stay on the device: the detector and the matching are two launches
    (..detector.score_on_device) and three integers per (keyword, threshold) come back instead of the event lists.  numpy input on a
    host without a GPU loops over detect() and tpr_fpr."""
    import torch
    from .tpr_fpr import tpr_fpr
    thresholds = list(thresholds)
    inferences, on_device, single, keywords = _keyword_planes(inferences, flags, keywords)
    N = inferences.shape[0]
    tol = flags.time_tolerance_ms
    if not tol >= 0:
        raise ValueError("time_tolerance_ms must be >= 0")
    gt = _groundtruth_times(groundtruth, keywords)
    if not all(np.isfinite(np.asarray(g, dtype=np.float64)).all() for g in gt):
        raise ValueError("ground-truth times must be finite")
    clip, stride, offsets = _stream_windows(inferences, flags, sample_rate, data_samples)
    if duration_s is None:
        duration_s = (data_samples if data_samples is not None else (inferences.shape[1] - 1) * stride + clip) / sample_rate
    capped = 0
    if not on_device and not torch.cuda.is_available():
        import contextlib
        import dataclasses
        import io
        curves = []
        said = io.StringIO()
        for n in range(N):
            kw_flags = dataclasses.replace(flags, target_keyword=keywords[n])
            curve = []
            for thr in thresholds:
                found = detect(inferences[n], kw_flags, thr, sample_rate, data_samples)[0]
                with contextlib.redirect_stdout(said):
                    curve.append(tpr_fpr(keywords[n], thr, found, gt[n], duration_s, tol, num_nontarget_words))
            curves.append(curve)
        capped = said.getvalue().count("WARNING: weird timing issue")
    else:
        if len(flags.labels()) != inferences.shape[2]:
            raise ValueError("The results for recognition should contain {} elements, but there are {} produced".format(
                len(flags.labels()), inferences.shape[2]))
        from ..detector import score_on_device
        t_ms = [int(off * 1000 / sample_rate) for off in offsets]
        curves = [[] for _ in range(N)]
        if thresholds:
            tally = score_on_device(inferences[:, :len(offsets)], t_ms, thresholds, gt, tol, flags.average_window_duration_ms,
                                    flags.suppression_ms, flags.minimum_count, target_id=2).tolist()
            for n in range(N):
                curves[n], was_capped = _curve_from_tally(keywords[n], thresholds, tally[n], len(gt[n]), duration_s, num_nontarget_words)
                capped += was_capped
    if capped:
        print(f"WARNING: weird timing issue ({capped} of {N * len(thresholds)} keyword x threshold lanes: true positives capped to the ground-truth count)")
    return curves[0] if single else curves


def _shared_embedding_passes(keywords, models, wav, groundtruth, thresholds, inference_chunk_len_seconds, average_window_duration_ms,
                             suppression_ms, time_tolerance_ms, resample=False, channel=0):
    """What multi_keyword_detections and multi_keyword_operating_curves do with a recording before their detector runs: the argument
    checks and the wav are done when this returns -> (keywords as a list, the StreamFlags of the run, sample rate, samples of the
    recording, an iterator over the distinct embeddings of `models` that yields (indices of the models on it, their softmax outputs
    [len(indices), windows, 3] on the device): one streaming_inferences pass each).  resample=True: a recording at another rate than the
    model's is converted on the device first (input_data.to_sample_rate, centred); rate and samples are then the converted audio's.
    With resample=True the recording may have any supported WAV format and `channel` (an int, or "mix") selects what is heard: it is
    read by input_data.read_recording, unless it is the first channel of a 16-bit PCM file at the model's rate, which is decoded on the
    host as before.  The default path reads the first channel of a 16-bit PCM file and takes no other channel."""
    keywords, models = list(keywords), list(models)
    if len(models) != len(keywords) or len(set(keywords)) != len(keywords):
        raise ValueError(f"discrepancy: {len(models)} models provided for {len(set(keywords))} keywords")
    if inference_chunk_len_seconds <= 0:
        raise ValueError("inference_chunk_len_seconds must be positive")
    model_settings = input_data.standard_microspeech_model_settings(label_count=3)
    if not resample and channel != 0:
        raise ValueError(f"channel={channel!r} needs resample=True: the default path reads the first channel of a 16-bit PCM file")
    with open(wav, "rb") as f:
        image = f.read()
    if resample:
        from .. import pcm
        info = pcm.wav_info(image)
    if resample and (info.rate != model_settings["sample_rate"] or info.format != "s16" or channel != 0):
        sample_rate = model_settings["sample_rate"]
        audio = input_data.read_recording(image, sample_rate, channel)                # decoded and converted on the device, stays there
    else:                                                                             # nothing to convert: taken as it is, as before
        audio, sample_rate = input_data.decode_wav(image)
    flags = StreamFlags(wav=wav, ground_truth=groundtruth, target_keyword=keywords[0] if keywords else "", detection_thresholds=thresholds,
                        average_window_duration_ms=average_window_duration_ms, suppression_ms=suppression_ms,
                        time_tolerance_ms=time_tolerance_ms, max_chunk_length_sec=inference_chunk_len_seconds)
    by_embedding = {}
    for i, m in enumerate(models):                                  # one pass per distinct embedding (normally one)
        by_embedding.setdefault(id(m.embedding), []).append(i)

    def passes():
        for idxs in by_embedding.values():
            yield idxs, streaming_inferences([models[i] for i in idxs], model_settings, audio, sample_rate, 1000, 20,
                                             max_chunk_length_sec=inference_chunk_len_seconds, as_device=True)
    return keywords, flags, sample_rate, audio.shape[0], passes()


def multi_keyword_operating_curves(keywords, models, wav, groundtruth_csv, thresholds, inference_chunk_len_seconds=1200,
                                   average_window_duration_ms=100, suppression_ms=500, time_tolerance_ms=750, num_nontarget_words=None,
                                   resample=False, channel=0):
    """From a recording to {keyword: [tpr_fpr's dict per threshold]} for N keywords: one pass over the wav on the shared embedding
    (streaming_inferences(as_device=True), as multi_keyword_detections), then operating_curves on the device tensor -- the probabilities,
    the detections and the matching never visit the host.  groundtruth_csv: rows `keyword,time_ms` (run.py's ground-truth file).  The
    other arguments are multi_keyword_detections' flags (resample and channel too); the recording's duration is its sample count over its
    sample rate."""
    thresholds = list(thresholds)
    keywords, flags, sample_rate, data_samples, passes = _shared_embedding_passes(
        keywords, models, wav, groundtruth_csv, thresholds, inference_chunk_len_seconds, average_window_duration_ms, suppression_ms, time_tolerance_ms,
        resample=resample, channel=channel)
    groundtruth_data = _read_groundtruth(groundtruth_csv)
    curves = {}
    for idxs, got in passes:
        per = operating_curves(got, flags, thresholds, groundtruth_data, keywords=[keywords[i] for i in idxs], sample_rate=sample_rate,
                               data_samples=data_samples, num_nontarget_words=num_nontarget_words)
        for i, curve in zip(idxs, per):
            curves[keywords[i]] = curve
    return {kw: curves[kw] for kw in keywords}


def _one_recording(flag_list):
    """What the StreamFlags of one target must share: one wav, one clip length, one stride."""
    assert len(set([f.wav for f in flag_list])) == 1, "can only process one wav"
    assert len(set([f.clip_duration_ms for f in flag_list])) == 1, "cannot vary"
    assert len(set([f.clip_stride_ms for f in flag_list])) == 1, "cannot vary"


def calculate_streaming_accuracy(model, model_settings, flag_list, existing_inferences=None):
    """Reference signature (:50-179): one wav, several StreamFlags; returns (results, inferences) with
    results = [(FLAGS, {threshold: (found_words, found_words_w_confidences)})]."""
    _one_recording(flag_list)
    with open(flag_list[0].wav, "rb") as f:
        audio, sample_rate = input_data.decode_wav(f.read())
    if existing_inferences is not None:
        inferences = existing_inferences
    else:
        inferences = streaming_inferences(model, model_settings, audio, sample_rate, flag_list[0].clip_duration_ms,
                                          flag_list[0].clip_stride_ms, max_chunk_length_sec=flag_list[0].max_chunk_length_sec, as_device=True)
    import torch
    dev_inferences = inferences                                      # what the detector reads: the device copy where there is a device
    if torch.is_tensor(inferences):
        inferences = inferences.cpu().numpy()
    elif torch.cuda.is_available():
        dev_inferences = torch.from_numpy(np.ascontiguousarray(inferences)).cuda()
    results = []
    for FLAGS in flag_list:                                          # all thresholds of a StreamFlags in one launch
        results.append((FLAGS, detect_many(dev_inferences, FLAGS, FLAGS.detection_thresholds, sample_rate, data_samples=audio.shape[0])))
    return results, inferences


@dataclass
class StreamTarget:
    """Reference :188-195 -- one keyword's streaming evaluation: where its model is, what to run it on, where results go."""
    target_lang: str
    target_word: str
    model_path: os.PathLike
    stream_flags: List[StreamFlags]
    destination_result_pkl: Optional[os.PathLike] = None
    destination_result_inferences: Optional[os.PathLike] = None


def eval_stream_test(st: StreamTarget, live_model=None):
    """Reference :198-241.  -> {target_word: [(FLAGS, {threshold: (found_words, found_words_w_confidences)}), ...]}, or None (after a
    message) when destination_result_pkl already exists.  The model is `live_model` or TransferLearnedModel.load(st.model_path) (the
    directory transfer_learn's model.save() wrote -- the counterpart of tf.keras.models.load_model).  Results are pickled to
    destination_result_pkl and the raw per-window softmax outputs saved (np.save) to destination_result_inferences when those are
    given; inferences found there are re-used instead of being recomputed.  (The reference reads them back from the PICKLE path --
    np.load(st.destination_result_pkl), a file it has just established does not exist -- so its re-use branch cannot run; here the
    branch loads the file it tested for.)"""
    if live_model is not None:
        model = live_model
    else:
        from .transfer_learning import TransferLearnedModel
        model = TransferLearnedModel.load(os.fspath(st.model_path))
    model_settings = input_data.standard_microspeech_model_settings(label_count=3)

    if st.destination_result_pkl is not None and os.path.isfile(st.destination_result_pkl):
        print("results already present", st.destination_result_pkl, flush=True)
        return
    loaded_inferences = None
    if st.destination_result_inferences is not None and os.path.isfile(st.destination_result_inferences):
        print("inferences already present", flush=True)
        loaded_inferences = np.load(st.destination_result_inferences)

    results = {}
    results[st.target_word], inferences = calculate_streaming_accuracy(model, model_settings, st.stream_flags, loaded_inferences)

    if st.destination_result_pkl is not None:
        print("SAVING results TO\n", st.destination_result_pkl)
        with open(st.destination_result_pkl, "wb") as fh:
            pickle.dump(results, fh)
    if loaded_inferences is None and st.destination_result_inferences is not None:
        print("SAVING inferences TO\n", st.destination_result_inferences, flush=True)
        np.save(st.destination_result_inferences, inferences)
    return results


def multi_keyword_detections(keywords, models, wav, detection_threshold=0.9, inference_chunk_len_seconds=1200, groundtruth=None,
                             average_window_duration_ms=100, suppression_ms=500, write_detections=None, resample=False, channel=0):
    """The detections dict of run.py:89-152 for N keywords from ONE pass over the recording.

    The reference loads one full Keras model per keyword and repeats the window loop, the micro-frontend and the EfficientNet forward
    for each (one child process per keyword); here `models` (TransferLearnedModels sharing one embedding, transfer_learning.
    load_models_shared) are N 18.5 k-parameter heads on one embedding pass (streaming_inferences), and every keyword's detector runs over
    its own head's outputs in one launch (detect_many).  Per keyword the detections are exactly what eval_stream_test yields for StreamFlags(detection_thresholds=
    [detection_threshold], average_window_duration_ms=100, suppression_ms=500, max_chunk_length_sec=inference_chunk_len_seconds);
    they are merged and sorted by time (stable, like the reference's sorted()).  -> dict(keywords=..., detections=[dict(keyword, time_ms,
    confidence, groundtruth)], min_threshold=...): groundtruth "ng" without a ground-truth file, otherwise tpr_fpr.get_groundtruth's
    classification against its rows `keyword,time_ms` (as shipped: first keyword only).  Also written as JSON to write_detections.
    resample=True: a recording whose rate differs from the model's 16 kHz is converted on the device (resample.Resampler, centred) before
    windowing, and the times are those of the converted audio; with the default the recording is taken as it is.  With resample=True the
    file may have any supported WAV format and `channel` (an int, or "mix") selects which channel is heard."""
    import json
    keywords, flags, sample_rate, data_samples, passes = _shared_embedding_passes(
        keywords, models, wav, groundtruth, [detection_threshold], inference_chunk_len_seconds, average_window_duration_ms, suppression_ms, 750,
        resample=resample, channel=channel)
    per_keyword = [None] * len(keywords)                            # keyword -> its found_words_w_confidences
    for idxs, got in passes:
        found = detect_many(got, flags, [detection_threshold], sample_rate, data_samples=data_samples, keywords=[keywords[i] for i in idxs])
        for i, by_threshold in zip(idxs, found):
            per_keyword[i] = by_threshold[detection_threshold][1]
    unsorted_detections = []
    for found_conf in per_keyword:
        unsorted_detections.extend(found_conf)
    detections_with_confidence = sorted(unsorted_detections, key=lambda d: d[1])
    if groundtruth is None:
        detections_with_confidence = [dict(keyword=d[0], time_ms=d[1], confidence=d[2], groundtruth="ng") for d in detections_with_confidence]
    else:
        from .tpr_fpr import get_groundtruth
        detections_with_confidence = get_groundtruth(detections_with_confidence, keywords, _read_groundtruth(groundtruth))
    detections = dict(keywords=keywords, detections=detections_with_confidence, min_threshold=detection_threshold)
    if write_detections is not None:
        with open(write_detections, "w") as fh:
            json.dump(detections, fh)
    return detections


# ---------------------------------------------------------------------------------------------------------------------------------
# The batch entry point (reference :244-337): K (keyword, recording) pairs -- every target its own recording, its own fine-tuned head and
# its own ground truth -- in one device pass instead of one eval_stream_test after the other.


class _Prepared:
    """One StreamTarget of a batch pass: its recording, the rows its inferences take in the pass's [rows, 3] tensor, and what is known
    about them so far."""

    def __init__(self, index, st):
        self.index, self.st = index, st
        self.audio = self.sample_rate = self.loaded = self.inferences = self.model = None
        self.rows = self.base = 0
        self.plain = True               # float32 [rows, 3] inferences: the target's rows live in the shared device tensor


def _read_target(p, live_model):
    """What calculate_streaming_accuracy establishes before it runs anything: one wav, one clip length, one stride."""
    flag_list = p.st.stream_flags
    _one_recording(flag_list)
    with open(flag_list[0].wav, "rb") as f:
        p.audio, p.sample_rate = input_data.decode_wav(f.read())
    p.model = live_model
    f0 = flag_list[0]
    p.clip = int(f0.clip_duration_ms * p.sample_rate / 1000)
    p.stride = int(f0.clip_stride_ms * p.sample_rate / 1000)
    p.offsets = window_offsets(p.audio.shape[0], p.clip, p.stride)
    if p.loaded is not None:
        a = np.asarray(p.loaded)
        p.inferences = a
        p.plain = a.ndim == 2 and a.shape[1] == 3 and a.dtype == np.float32
        p.rows = a.shape[0] if p.plain else 0
    else:
        max_chunk = None if f0.max_chunk_length_sec is None else int(f0.max_chunk_length_sec * p.sample_rate)
        p.chunks = chunk_audio(p.audio, max_chunk)
        p.rows = sum(max(0, len(window_offsets(c.shape[0], p.clip, p.stride))) for c in p.chunks)


def _batch_inferences(prepared):
    """The softmax outputs of every prepared target in ONE device tensor [rows, 3] (target p at rows p.base .. p.base + p.rows): stored
    inferences are uploaded into their rows; the other targets are grouped by (embedding handle, head dimensions, clip length, stride,
    sample rate) and each group is one pass -- the recordings windowed one after the other (chunk_audio as shipped, per recording), the
    windows packed into full batches of the handle's max_batch regardless of recording boundaries, the embedding run eagerly on the
    caller's handle and HeadGroup.forward_segments writing each batch's probabilities under the head of the recording each row belongs to.
    Device memory: one recording's spectrograms, one batch of embeddings, 12 bytes per row.  Sets p.inferences (host) for every target;
    -> the device tensor, or None on a host without a GPU (then every target must have come with stored inferences)."""
    import torch
    from ..head import HeadGroup
    at = 0
    for p in prepared:
        p.base, at = at, at + p.rows
    todo = [p for p in prepared if p.loaded is None]
    if not torch.cuda.is_available() and not todo:
        return None
    groups = {}
    for p in todo:
        hd = p.model.head
        key = (id(p.model.embedding), hd.in_dim, hd.hidden, hd.classes, p.clip, p.stride, p.sample_rate)
        groups.setdefault(key, []).append(p)
    dev = todo[0].model.embedding.device if todo else torch.device(f"cuda:{torch.cuda.current_device()}")
    d_all = torch.empty((at, 3), dtype=torch.float32, device=dev)
    for p in prepared:
        if p.loaded is not None and p.plain and p.rows:
            d_all[p.base:p.base + p.rows].copy_(torch.from_numpy(np.ascontiguousarray(p.inferences)), non_blocking=True)
    model_settings = input_data.standard_microspeech_model_settings(label_count=3)
    for members in groups.values():
        emb_model = members[0].model.embedding
        if members[0].model.head.classes != 3:
            raise ValueError("The results for recognition should contain 3 elements, but there are {} produced".format(members[0].model.head.classes))
        if emb_model.device != dev:
            raise ValueError("eval_stream_tests: the targets' embeddings live on different devices")
        heads, slot = [], {}
        for p in members:                                           # a head shared by several targets is one member of the group
            if id(p.model.head) not in slot:
                slot[id(p.model.head)] = len(heads)
                heads.append(p.model.head)
        seg_off = np.zeros(len(members) + 1, np.int64)
        np.cumsum([p.rows for p in members], out=seg_off[1:])
        if seg_off[-1] == 0:
            continue
        if seg_off[-1] >= 2 ** 31:
            raise ValueError("too many windows for one pass")
        mb, dim = emb_model.max_batch, emb_model.output_dim
        rows = int(seg_off[-1])
        group = HeadGroup(heads)
        try:
            with torch.cuda.device(dev):
                d_off = torch.from_numpy(seg_off.astype(np.int32)).to(dev)
                d_head = torch.tensor([slot[id(p.model.head)] for p in members], dtype=torch.int32, device=dev)
                contiguous = all(a.base + a.rows == b.base for a, b in zip(members, members[1:]))
                d_probs = d_all[members[0].base:members[0].base + rows] if contiguous else torch.empty((rows, 3), dtype=torch.float32, device=dev)

                def one_pass():
                    d_emb = torch.empty((min(mb, rows), dim), dtype=torch.float32, device=dev)
                    d_bad = torch.zeros((rows + mb - 1) // mb, dtype=torch.int32, device=dev)
                    carry, done = None, 0

                    def run(spec):
                        nonlocal done
                        r = spec.shape[0]
                        emb_model.forward(spec, out=d_emb[:r])
                        group.forward_segments(d_emb[:r], d_off, d_head, row_base=done, out=d_probs[done:done + r], invalid=d_bad[done // mb:done // mb + 1])
                        done += r
                    for p in members:
                        for chunk in p.chunks:
                            specs = stream_spectrograms(model_settings, chunk, p.clip, p.stride)
                            if specs.shape[0] == 0:
                                continue
                            if carry is not None:
                                specs = torch.cat([carry, specs])
                            full = specs.shape[0] // mb * mb
                            for s in range(0, full, mb):
                                run(specs[s:s + mb])
                            carry = specs[full:].clone() if full < specs.shape[0] else None     # (a copy: the recording's spectrograms are released)
                    if carry is not None:
                        run(carry)
                    assert done == rows, (done, rows)
                    return d_probs.cpu().numpy(), int(d_bad.sum().cpu())
                host, n_bad = emb_model.checked(one_pass)
        finally:
            group.close()
        if n_bad:
            raise RuntimeError(f"{n_bad} windows reached the device outside every recording's rows")
        for i, p in enumerate(members):
            p.inferences = host[int(seg_off[i]):int(seg_off[i + 1])]
            if not contiguous and p.rows:
                d_all[p.base:p.base + p.rows].copy_(d_probs[int(seg_off[i]):int(seg_off[i + 1])])
    return d_all


def _detector_segments(prepared, d_all, keyed):
    """The (target, StreamFlags) pairs of a pass grouped by `keyed(flags)`, each group with what one segmented detector call needs:
    -> {key: (pairs [(p, flags)], probs [rows, 3] on the device, offsets [S + 1], times [rows])}.  A segment is the target's rows cut to
    its window offsets (chunk_audio as shipped can yield more rows than offsets: detect_many cuts them too); fewer rows raise IndexError."""
    import torch
    by_key = {}
    for p in prepared:
        if not p.plain:
            continue
        for flags in p.st.stream_flags:
            if flags.detection_thresholds:
                by_key.setdefault(keyed(flags), []).append((p, flags))
    out = {}
    for key, pairs in by_key.items():
        spans, times = [], []
        for p, _ in pairs:
            n = len(p.offsets)
            if p.rows < n:
                raise IndexError(f"index {p.rows} is out of bounds: {p.rows} rows of inferences for {n} windows")
            spans.append((p.base, p.base + n))
            times.append(np.asarray([int(off * 1000 / p.sample_rate) for off in p.offsets], dtype=np.int64))
        off = np.zeros(len(pairs) + 1, np.int64)
        np.cumsum([b - a for a, b in spans], out=off[1:])
        whole = spans[0][0] == 0 and spans[-1][1] == d_all.shape[0] and all(a[1] == b[0] for a, b in zip(spans, spans[1:]))
        probs = d_all if whole else (torch.cat([d_all[a:b] for a, b in spans]) if spans else d_all[:0])
        out[key] = (pairs, probs, off, np.concatenate(times) if times else np.zeros(0, np.int64))
    return out


def _prepare(stream_targets, live_models, skip_done):
    targets = list(stream_targets)
    if live_models is not None:
        live_models = list(live_models)
        if len(live_models) != len(targets):
            raise ValueError(f"{len(live_models)} live models for {len(targets)} stream targets")
    prepared = []
    for i, st in enumerate(targets):
        if skip_done and st.destination_result_pkl is not None and os.path.isfile(st.destination_result_pkl):
            print("results already present", st.destination_result_pkl, flush=True)
            continue
        p = _Prepared(i, st)
        if st.destination_result_inferences is not None and os.path.isfile(st.destination_result_inferences):
            print("inferences already present", flush=True)
            p.loaded = np.load(st.destination_result_inferences)
        prepared.append(p)
    need = [p for p in prepared if p.loaded is None]
    if live_models is None and need:
        from .transfer_learning import load_models_shared
        for p, m in zip(need, load_models_shared([p.st.model_path for p in need])):
            p.model = m
    for p in prepared:
        _read_target(p, live_models[p.index] if live_models is not None else p.model)
    return targets, prepared


def _save_inferences(p):
    if p.loaded is None and p.st.destination_result_inferences is not None:
        print("SAVING inferences TO\n", p.st.destination_result_inferences, flush=True)
        np.save(p.st.destination_result_inferences, p.inferences)


def eval_stream_tests(stream_targets, live_models=None):
    """eval_stream_test for a list of StreamTargets in one device pass: -> a list aligned with the targets, entry i being exactly what
    eval_stream_test(stream_targets[i], live_models[i]) returns (None after its "results already present" message), with the same
    pickle and .npy files written and stored inferences re-used.  Models: `live_models` (aligned with the targets), or
    transfer_learning.load_models_shared over the model_paths of the targets that need one.

    Where eval_stream_test pays, per target, an embedding pass that ends in a ragged batch, an upload, a detector launch per StreamFlags
    and a synchronising copy for each, this is one embedding pass per (embedding handle, clip length, stride, sample rate) over full
    batches that ignore recording boundaries (_batch_inferences: each row under its own recording's head), and ONE
    detector.detect_segments_on_device call per distinct (average window, suppression, minimum count, thresholds) over all targets and
    flags.  No hipGraph and no serving lanes: the eager path of one handle is bit-identical across batch sizes, which is what makes the
    results equal eval_stream_test's.  On a host without a GPU targets whose inferences are all stored run through the host detect()
    loop, as in eval_stream_test; anything that needs an embedding fails as it does there."""
    import torch
    from ..detector import detect_segments_on_device
    targets, prepared = _prepare(stream_targets, live_models, skip_done=True)
    out = [None] * len(targets)
    d_all = _batch_inferences(prepared)
    by_pair = {}
    if d_all is not None:
        keyed = lambda f: (f.average_window_duration_ms, f.suppression_ms, f.minimum_count, tuple(f.detection_thresholds))   # noqa: E731
        for key, (pairs, probs, off, times) in _detector_segments(prepared, d_all, keyed).items():
            thresholds = list(key[3])
            res = detect_segments_on_device(probs, off, times, thresholds, key[0], key[1], key[2], target_id=2, fired_only=True)
            counts = res.counts.tolist()
            for s, (p, flags) in enumerate(pairs):
                by_pair[(p.index, id(flags))] = _found_by_threshold(flags.target_keyword, times[off[s]:off[s + 1]].tolist(), thresholds,
                                                                    res.event_buffer[s], counts[s])
    for p in prepared:
        per_flags = []
        for flags in p.st.stream_flags:
            found = by_pair.get((p.index, id(flags)))
            if found is None:             # no device, no thresholds, or stored inferences that are not float32 [rows, 3]: detect_many's own routes
                found = detect_many(p.inferences, flags, flags.detection_thresholds, p.sample_rate, data_samples=p.audio.shape[0])
            per_flags.append((flags, found))
        results = {p.st.target_word: per_flags}
        if p.st.destination_result_pkl is not None:
            print("SAVING results TO\n", p.st.destination_result_pkl)
            with open(p.st.destination_result_pkl, "wb") as fh:
                pickle.dump(results, fh)
        _save_inferences(p)
        out[p.index] = results
    return out


def stream_operating_curves(stream_targets, live_models=None, num_nontarget_words=None):
    """Per target and per StreamFlags the list of tpr_fpr dicts operating_curves gives for that target's inferences, its flags'
    thresholds and the ground truth in flags.ground_truth (rows `keyword,time_ms`; the recording's duration is its samples over its
    sample rate) -- from the pass of eval_stream_tests (stored inferences re-used, new ones saved; result pickles are neither read nor
    written) and ONE detector.score_segments_on_device call per distinct detector setting, thresholds and tolerance, summary_from_tally
    on three integers per lane.  A host without a GPU takes operating_curves' host route per target."""
    from ..detector import score_segments_on_device
    targets, prepared = _prepare(stream_targets, live_models, skip_done=False)
    d_all = _batch_inferences(prepared)
    gt_cache = {}

    def groundtruth(flags):
        path = os.fspath(flags.ground_truth)
        if path not in gt_cache:
            gt_cache[path] = _read_groundtruth(path)
        return gt_cache[path]
    by_pair, capped, lanes = {}, 0, 0
    if d_all is not None:
        keyed = lambda f: (f.average_window_duration_ms, f.suppression_ms, f.minimum_count, tuple(f.detection_thresholds), f.time_tolerance_ms)   # noqa: E731
        for key, (pairs, probs, off, times) in _detector_segments(prepared, d_all, keyed).items():
            thresholds = list(key[3])
            gts = [_groundtruth_times(groundtruth(flags), [flags.target_keyword])[0] for _, flags in pairs]
            tally = score_segments_on_device(probs, off, times, thresholds, gts, key[4], key[0], key[1], key[2], target_id=2).tolist()
            for s, (p, flags) in enumerate(pairs):
                by_pair[(p.index, id(flags))], was_capped = _curve_from_tally(flags.target_keyword, thresholds, tally[s], len(gts[s]),
                                                                              p.audio.shape[0] / p.sample_rate, num_nontarget_words)
                capped += was_capped
                lanes += len(thresholds)
    if capped:
        print(f"WARNING: weird timing issue ({capped} of {lanes} keyword x threshold lanes: true positives capped to the ground-truth count)")
    out = [None] * len(targets)
    for p in prepared:
        curves = []
        for flags in p.st.stream_flags:
            curve = by_pair.get((p.index, id(flags)))
            if curve is None:
                curve = operating_curves(p.inferences, flags, flags.detection_thresholds, groundtruth(flags), sample_rate=p.sample_rate,
                                         data_samples=p.audio.shape[0], num_nontarget_words=num_nontarget_words)
            curves.append(curve)
        _save_inferences(p)
        out[p.index] = curves
    return out


def batch_streaming_analysis(sse, dest_dir, detection_thresholds=None, shuffle=True, **flag_overrides):
    """Reference :244-337 with its two undefined globals as parameters: walks sse/<lang>/<word>/{model/<one entry>, streaming_test.wav,
    streaming_labels.txt}, builds one StreamTarget per keyword with results under dest_dir/<lang>/<word>/{stream_results.pkl,
    raw_inferences.npy} (ValueError "extra models or no models", AssertionError "missing stream info" / "result data already present",
    as there), shuffles them (np.random.shuffle, as there) unless shuffle=False, creates every result directory and evaluates them all
    with eval_stream_tests (the reference: one child process per target).  detection_thresholds: default np.linspace(0.05, 1, 20);
    flag_overrides: further StreamFlags fields.  -> (targets, results), aligned."""
    from pathlib import Path
    sse, dest_dir = Path(sse), Path(dest_dir)
    if detection_thresholds is None:
        detection_thresholds = np.linspace(0.05, 1, 20).tolist()       # step threshold 0.05
    batch_data_to_process = []
    for lang_dir in os.listdir(sse):
        if not os.path.isdir(sse / lang_dir):
            continue                                                   # skip the data generator shellscript and the logfiles
        target_lang = lang_dir.split("_")[-1]
        for word_dir in os.listdir(sse / lang_dir):
            target_word = word_dir.split("_")[-1]
            print(target_lang, target_word)
            model_files = os.listdir(sse / lang_dir / word_dir / "model")
            if len(model_files) != 1:
                raise ValueError("extra models or no models")
            model_path = sse / lang_dir / word_dir / "model" / model_files[0]
            stream_wav = sse / lang_dir / word_dir / "streaming_test.wav"
            stream_label = sse / lang_dir / word_dir / "streaming_labels.txt"
            assert os.path.isfile(stream_wav) and os.path.isfile(stream_label), "missing stream info"
            destination_result_pkl = dest_dir / lang_dir / word_dir / "stream_results.pkl"
            destination_result_inferences = dest_dir / lang_dir / word_dir / "raw_inferences.npy"
            assert not os.path.isfile(destination_result_pkl) and not os.path.isfile(destination_result_inferences), "result data already present"
            flags = StreamFlags(wav=str(stream_wav), ground_truth=str(stream_label), target_keyword=target_word,
                                detection_thresholds=list(detection_thresholds), **flag_overrides)
            batch_data_to_process.append(StreamTarget(target_lang=target_lang, target_word=target_word, model_path=model_path, stream_flags=[flags],
                                                      destination_result_pkl=destination_result_pkl,
                                                      destination_result_inferences=destination_result_inferences))
    if shuffle:
        np.random.shuffle(batch_data_to_process)
    print("n wavs", len(batch_data_to_process), flush=True)
    for d in batch_data_to_process:
        result_dir = os.path.split(d.destination_result_pkl)[0]
        print("making dir", result_dir, flush=True)
        os.makedirs(result_dir, exist_ok=True)
    return batch_data_to_process, eval_stream_tests(batch_data_to_process)
