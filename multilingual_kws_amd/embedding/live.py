"""Live serving: the detector run one window or one push at a time, as one captured chain of launches per call.

StreamingSession is the reference's window loop (batch_streaming_analysis.py:99-117) for the newest window; LiveSession keeps the frontend's
frames and the detector's state on the device and takes audio chunks of any length; LiveSessionGroup serves S such streams in lockstep and
LiveRoutedGroup gives every slot its own keywords.  All four replay their chain through _CapturedChain, which is where the warm-up, capture
and heal-and-recapture protocol is written; the two live forms share one device side, _LiveChain (the session is its one-row, maskless
instance).  batch_streaming_analysis re-exports every public name of this module."""
import numpy as np

from . import input_data
from ..detector import (detect_live_step_many, detect_live_step_routes, live_detector_state_many, live_detector_state_routes, live_history,
                        live_out_words_many, live_out_words_routes, live_unpack_many)
from ..frontend import live_window_time_ms, live_windows
from ..head import Head, HeadGroup
from ..resample import live_push_hops


class _CapturedChain:
    """A chain of launches run eagerly or replayed as one hipGraph.  The owner provides self.embedding, _chain() -> the chain's output
    tensor, and _chain_state(); this class owns .graph (None: eager), .recaptures and .probs (the output of the latest run: with a graph,
    the static output of the capture)."""

    def _chain_state(self):
        """The tensors a run of the chain advances: _capture puts them back.  None here (StreamingSession's chain is stateless)."""
        return []

    def _start(self, use_graph):
        self.graph = None
        self.recaptures = 0
        self.probs = self._chain()                      # eager pass: creates every lazily-built table / attribute
        if use_graph:
            self._capture()

    def _capture(self):
        """Warm-up (which heals a handle with a recorded exchange failure: the wrapper repeats the call) and capture, on a single stream:
        the chain is one branch.  The warm-up and the capture's own pass run a stateful chain: its state tensors are put back afterwards,
        so capturing advances no stream."""
        import torch
        dev = self.embedding.device
        states = self._chain_state()
        kept = [t.clone() for t in states]
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            self._chain()
        torch.cuda.current_stream(dev).wait_stream(side)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            self.probs = self._chain()
        self.graph = g
        for t, k in zip(states, kept):
            t.copy_(k)

    def _run(self):
        """One run of the chain on the current stream: a replay, or the eager chain without a graph."""
        if self.graph is None:
            self.probs = self._chain()
            return
        if self.embedding.get_option("exchange_error"):
            # the PREVIOUS replay ran a failed pair / cluster exchange (its probabilities were all-NaN, never plausible numbers: a live
            # detector scored NaN and reported no event; the frontend rings are unaffected); the captured launches would poison every
            # later window as well: heal the handle and capture the single-workgroup kernels
            self._capture()
            self.recaptures += 1
        self.graph.replay()


def _require_micro(model_settings, who):
    """The live chains are built on the micro frontend's live push: settings of another preprocess mode are refused (they used to be
    served micro features without a word).  -> the settings."""
    mode = model_settings.get("preprocess", "micro")
    if mode != "micro":
        raise ValueError(f'{who}: the live chain is micro-only, model_settings["preprocess"] is {mode!r} '
                         "(input_data.to_features and stream_spectrograms serve the mfcc and average modes)")
    return model_settings


def _embedding_and_heads(models, embedding, heads):
    """models: TransferLearnedModel(s) sharing one embedding, or None for embedding= and heads= as they are -> (embedding, [heads])."""
    if models is not None:
        mlist = list(models) if isinstance(models, (list, tuple)) else [models]
        embedding, heads = mlist[0].embedding, [m.head for m in mlist]
    return embedding, list(heads)


class StreamingSession(_CapturedChain):
    """Live serving of the reference's window loop (batch_streaming_analysis.py:99-117), one or a few windows at a time: the
    newest `batch` one-second windows -> micro-frontend -> embedding -> every keyword head, as ONE hipGraph replay.

    At batch 1 the path is ~65 small launches; issued one by one each costs a host round trip, so a window took 0.55 ms with
    the GPU mostly idle.  All mkws_* calls are asynchronous, allocation-free and synchronisation-free on the caller's stream
    (include/mkws.h), so the whole chain is captured once and replayed: the per-window host cost is one copy into the static
    input and one graph launch.  Results are the same launches on the same buffers, i.e. bit-identical to the eager calls.

    models: TransferLearnedModel(s) sharing one embedding (or pass embedding= and heads= directly)."""

    def __init__(self, models=None, model_settings=None, batch=1, embedding=None, heads=None, use_graph=True):
        import torch
        self.embedding, self.heads = _embedding_and_heads(models, embedding, heads)
        self.batch = int(batch)
        if self.batch > self.embedding.max_batch:
            raise ValueError(f"StreamingSession(batch={batch}) exceeds the embedding handle's max_batch={self.embedding.max_batch}")
        ms = _require_micro(model_settings or input_data.standard_microspeech_model_settings(3), "StreamingSession")
        self.samples = ms["desired_samples"]
        self.fe = input_data._frontend_for(ms, self.samples)
        self.audio = torch.zeros((self.batch, self.samples), dtype=torch.float32, device=self.embedding.device)      # static graph input
        self._start(use_graph)

    def _chain(self):
        if self.batch == 1:
            # one window: the frame-parallel streaming kernels (49 frames on 49 waves across the chip, then the window's scan) instead of
            # the batch kernel's one workgroup walking the 49 frames four at a time: 36 -> ~10 us; bit-identical (tests/test_frontend_gpu.py)
            spec = self.fe.stream(self.audio[0], self.samples, self.samples)
        else:
            spec = self.fe.forward(self.audio)
        return Head.forward_many(self.heads, self.embedding.forward(spec))

    def infer(self, audio):
        """audio: [samples] or [batch, samples] float32 (numpy, CPU or CUDA tensor) -> CUDA tensor [n_heads, batch, 3] of softmax
        outputs (a view of the session's static output: valid until the next infer)."""
        import torch
        a = audio if torch.is_tensor(audio) else torch.from_numpy(np.ascontiguousarray(audio, dtype=np.float32))
        self.audio.copy_(a.reshape(self.batch, self.samples), non_blocking=True)
        self._run()
        return self.probs


class LivePushCutter:
    """The host part of LiveSession.feed: chunks of any length -> whole pushes of `push_samples` samples; what does not fill a push
    waits for the next chunk.  The pushes depend on the samples fed so far only, not on how they were cut into chunks.  pcm16 (the
    sessions set it with input_rate): an int16 chunk is PCM and is taken as s / 32768, which is exact; without it every chunk is cast
    to float32 as it is."""

    def __init__(self, push_samples, pcm16=False):
        self.push_samples, self.pcm16 = int(push_samples), bool(pcm16)
        self.reset()

    def reset(self):
        self.rest = np.zeros(0, np.float32)

    def cut(self, chunk):
        """float32 samples -> [full pushes, push_samples] (a view of a fresh array; may have zero rows)."""
        if self.pcm16 and np.asarray(chunk).dtype == np.int16:
            a = (np.asarray(chunk).astype(np.float32) / np.float32(32768.0)).reshape(-1)
        else:
            a = np.asarray(chunk, dtype=np.float32).reshape(-1)
        if self.rest.size:
            a = np.concatenate([self.rest, a])
        full = a.size // self.push_samples
        self.rest = a[full * self.push_samples:].copy()
        return a[:full * self.push_samples].reshape(full, self.push_samples)


class LiveGroupScheduler:
    """The host part of LiveSessionGroup.feed: chunks of any length for some of `streams` slots -> ticks.  One LivePushCutter per slot;
    a tick is (active int32 [S], audio float32 [S, push_samples]): slot s is active in a tick if it has a whole push pending, and its row
    then holds that push (the rows of the others are zeros and are not read).  feed() emits ticks while any slot has a push, so nothing
    but the cutters' unfinished pushes waits between calls: tick t of a feed holds the t-th push each slot completed in it.  What a slot
    pushes depends only on the samples fed to THAT slot so far, never on how they were cut into chunks or on the other slots."""

    def __init__(self, streams, push_samples, pcm16=False):
        self.streams, self.push_samples = int(streams), int(push_samples)
        if self.streams < 1 or self.push_samples < 1:
            raise ValueError(f"LiveGroupScheduler({streams}, {push_samples}): at least one slot and one sample per push")
        self.cutters = [LivePushCutter(self.push_samples, pcm16) for _ in range(self.streams)]

    def reset(self, slot=None):
        for c in (self.cutters if slot is None else [self.cutters[self.slot(slot)]]):
            c.reset()

    def slot(self, slot):
        if not 0 <= int(slot) < self.streams:
            raise ValueError(f"slot {slot}: from 0 to {self.streams - 1}")
        return int(slot)

    def pending(self, slot):
        """Samples of the slot's unfinished push."""
        return int(self.cutters[self.slot(slot)].rest.size)

    def chunks(self, chunks):
        """{slot: samples} or a length-S sequence with None for silent slots -> [(slot, samples)] in slot order."""
        if isinstance(chunks, dict):
            items = sorted((self.slot(k), v) for k, v in chunks.items())
        else:
            chunks = list(chunks)
            if len(chunks) != self.streams:
                raise ValueError(f"{len(chunks)} chunks for {self.streams} slots (a dict {{slot: samples}} names some of them)")
            items = list(enumerate(chunks))
        return [(k, v) for k, v in items if v is not None]

    def feed(self, chunks):
        """-> the list of ticks these chunks complete (may be empty)."""
        pushes = {k: self.cutters[k].cut(v) for k, v in self.chunks(chunks)}
        ticks = []
        for t in range(max([len(v) for v in pushes.values()], default=0)):
            active = np.zeros(self.streams, np.int32)
            audio = np.zeros((self.streams, self.push_samples), np.float32)
            for k, v in pushes.items():
                if t < len(v):
                    active[k], audio[k] = 1, v[t]
            ticks.append((active, audio))
        return ticks


def default_live_flags(thresholds):
    from .batch_streaming_analysis import StreamFlags        # (at the call: that module imports this one)
    return StreamFlags(wav="", ground_truth="", target_keyword="", detection_thresholds=list(thresholds))


def _fed_samples(chunk):
    """A chunk as feed() takes it -> numpy on the host; a tensor comes as float32, or as int16 if it is that (the cutters decide what an
    int16 chunk means)."""
    import torch
    if torch.is_tensor(chunk):
        chunk = chunk.detach().reshape(-1)
        return chunk.to("cpu").numpy() if chunk.dtype == torch.int16 else chunk.to("cpu", torch.float32).numpy()
    return chunk


class _LiveChain(_CapturedChain):
    """The device side LiveSession and LiveSessionGroup share: `streams` rows of frontend, detector and (with input_rate) resampler state
    in device tensors (fstates, dstates, rstates: a row is a one-stream state block), the static buffers of one push of every row, and
    the chain over them,
        Resampler.live_push_many (with input_rate) -> Frontend.live_push_many -> embedding.forward -> Head.forward_many
        -> detect_live_step_many,
    run through _CapturedChain.  masked: the rows have an active mask that is uploaded with the audio, and a run pushes the active rows
    (the group).  Without one the calls get active=None and a run pushes every row: for one row that is what the library's one-stream
    entry points launch, argument for argument (the session)."""

    def __init__(self, models, streams, thresholds, flags, model_settings, hops_per_push, embedding, heads, keywords, fired_only, input_rate,
                 masked):
        import torch
        self._resolve(models, embedding, heads, streams, hops_per_push)
        ms = self._setup(thresholds, flags, model_settings, keywords, fired_only)
        self._input(input_rate)
        dev = self.embedding.device
        S, N, T, h = self.streams, len(self.heads), len(self.thresholds), self.hops
        with torch.cuda.device(dev):
            self._slot_buffers(ms, masked)
            self.dstates = live_detector_state_many(S, N, T, self.history, device=dev)
            self.d_thr = torch.tensor(self.thresholds, dtype=torch.float64, device=dev)
            self._out_buffers(live_out_words_many(S, N, T, h))

    def _resolve(self, models, embedding, heads, streams, hops_per_push):
        """models (or embedding= and heads=), the rows and the hops of a push -> self.embedding, .heads, .streams, .hops."""
        self.embedding, self.heads = _embedding_and_heads(models, embedding, heads)
        self.hops, self.streams = int(hops_per_push), int(streams)
        if self.streams < 1 or not 1 <= self.hops or self.streams * self.hops > self.embedding.max_batch:
            raise ValueError(f"{type(self).__name__}(streams={streams}, hops_per_push={hops_per_push}): streams * hops_per_push from 1 to the "
                             f"embedding handle's max_batch={self.embedding.max_batch}")

    def _setup(self, thresholds, flags, model_settings, keywords, fired_only):
        """What is derived from the arguments once embedding, heads and hops are set: thresholds, flags, keywords, the stream's geometry,
        the detector's history and the frontend handle.  -> the model settings."""
        self.thresholds = [float(t) for t in thresholds]
        if not self.thresholds:
            raise ValueError("at least one threshold")
        self.flags = flags if flags is not None else default_live_flags(self.thresholds)
        N = len(self.heads)
        if keywords is None:
            keywords = [self.flags.target_keyword or f"keyword_{i}" for i in range(N)]
        self.keywords = list(keywords)
        if len(self.keywords) != N:
            raise ValueError(f"{len(self.keywords)} keywords for {N} heads")
        return self._geometry(model_settings, fired_only)

    def _geometry(self, model_settings, fired_only):
        """The part of _setup that does not depend on who owns thresholds and keywords (LiveRoutedGroup: the routes do): from
        self.flags, self.heads and self.hops the stream's geometry, the detector's history and the frontend handle.  -> the model settings."""
        if self.heads[0].classes != len(self.flags.labels()):
            raise ValueError("The results for recognition should contain {} elements, but there are {} produced".format(
                len(self.flags.labels()), self.heads[0].classes))
        self.fired_only = bool(fired_only)
        ms = _require_micro(model_settings or input_data.standard_microspeech_model_settings(3), type(self).__name__)
        self.sample_rate = ms["sample_rate"]
        self.window_samples = int(self.flags.clip_duration_ms * self.sample_rate / 1000)
        self.hop_samples = int(self.flags.clip_stride_ms * self.sample_rate / 1000)
        self.push_samples = self.hops * self.hop_samples
        self.history = live_history(self.flags.average_window_duration_ms, self.hop_samples, self.sample_rate)
        self.fe = input_data._frontend_for(ms, self.window_samples)
        return ms

    def _input(self, input_rate):
        """The input side, once _geometry has run: self.in_push_samples, the samples of one push as the caller feeds
        them.  input_rate None or the model's own rate: the push itself, and nothing else changes (no .resampler attribute, the same chain).
        Otherwise self.resampler converts on the device, first launch of the chain, and a push of push_samples model-rate samples takes
        live_in_samples(push_samples) fed ones -- ValueError naming the smallest hops_per_push when that is not a whole number."""
        self.input_rate = self.sample_rate if input_rate is None else int(input_rate)
        self.in_push_samples = self.push_samples
        if self.input_rate == self.sample_rate:
            return
        if self.input_rate < 1:
            raise ValueError(f"input_rate={input_rate}")
        need = live_push_hops(self.input_rate, self.sample_rate, self.hop_samples)
        if self.hops % need:
            raise ValueError(f"input_rate={self.input_rate}: a push of {self.hops} hop(s) of {self.hop_samples} samples at {self.sample_rate} Hz is "
                             f"{self.push_samples * self.input_rate / self.sample_rate:g} input samples, not a whole number; the smallest "
                             f"hops_per_push that works is {need} (and its multiples)")
        self.resampler = input_data._resampler_for(self.input_rate, self.sample_rate, self.embedding.device)    # shared, never closed here
        self.in_push_samples = self.resampler.live_in_samples(self.push_samples)

    def _slot_buffers(self, ms, masked=True):
        """The per-row device buffers of a push and the pinned mirror of its one upload."""
        import torch
        dev, S, h, P = self.embedding.device, self.streams, self.hops, self.in_push_samples
        M = S if masked else 0
        # the static graph input, ONE buffer so that a push is one upload: the NEW samples [S, push] (float32), then the active mask [S] (int32)
        self.d_in = torch.zeros(S * P + M, dtype=torch.float32, device=dev)
        self.audio, self.active = self.d_in[:S * P].view(S, P), self.d_in[S * P:].view(torch.int32) if masked else None
        if hasattr(self, "resampler"):
            # the samples uploaded are the fed ones; the frontend's input is what the resampler writes
            self.raw, self.audio = self.audio, torch.zeros((S, self.push_samples), dtype=torch.float32, device=dev)
            self.rstates = self.resampler.live_state_many(S, device=dev)
        self.fstates = self.fe.live_state_many(S, self.window_samples, self.hop_samples, h, device=dev)
        self.spec = torch.zeros((S * h, ms["spectrogram_length"], ms["fingerprint_width"]), dtype=torch.float32, device=dev)
        self.meta = torch.zeros((S, 2 + h), dtype=torch.int64, device=dev)
        self.h_in = torch.zeros(S * P + M, dtype=torch.float32).pin_memory()
        self.h_audio, self.h_active = self.h_in[:S * P].view(S, P).numpy(), self.h_in[S * P:].view(torch.int32).numpy()

    def _out_buffers(self, words):
        import torch
        self.out = torch.zeros(words, dtype=torch.int64, device=self.embedding.device)   # counts and events: the one D2H per push
        self.h_out = torch.zeros(words, dtype=torch.int64).pin_memory()

    def _chain_state(self):
        return [self.fstates, self.dstates] + ([self.rstates] if hasattr(self, "resampler") else [])

    def _frontend_push(self):
        """The head of the chain: with input_rate the fed samples of every active row -> self.audio, then the frontend push of those rows."""
        if hasattr(self, "resampler"):
            self.resampler.live_push_many(self.rstates, self.raw, self.push_samples, active=self.active, out=self.audio)
        self.fe.live_push_many(self.fstates, self.audio, self.window_samples, self.hop_samples, self.hops, active=self.active,
                               spec=self.spec, meta=self.meta)

    def _chain(self):
        f = self.flags
        self._frontend_push()
        probs = Head.forward_many(self.heads, self.embedding.forward(self.spec))
        detect_live_step_many(self.dstates, probs, self.meta, self.d_thr, f.average_window_duration_ms, f.suppression_ms, f.minimum_count,
                              self.history, target_id=2, fired_only=self.fired_only, out=self.out)
        return probs

    def _before_replay(self):
        """Hook between a push's upload and its replay, on the same stream (LiveRoutedGroup uploads its edited tables here)."""

    def _roundtrip(self):
        """The device part of one push, h_in filled: one upload, one replay (or the eager chain), one download into h_out, one synchronise."""
        import torch
        dev = self.embedding.device
        with torch.cuda.device(dev):
            self.d_in.copy_(self.h_in, non_blocking=True)
            self._before_replay()
            self._run()
            self.h_out.copy_(self.out, non_blocking=True)
            torch.cuda.current_stream(dev).synchronize()

    def _unpack(self, first):
        """h_out after a push -> {row: records (window, head, threshold index, fired, score)} of the events it completed, in no order;
        first: {row: index of its first new window}."""
        counts, events = live_unpack_many(self.h_out.numpy(), self.streams, len(self.heads), len(self.thresholds), self.hops)
        fresh = {}
        if counts.any():
            for s, n, k in zip(*np.nonzero(counts)):
                for w, fired, score in events[s, n, k, :counts[s, n, k]].tolist():
                    fresh.setdefault(int(s), []).append((first[int(s)] + w, int(n), int(k), fired, score))
        return fresh

    def _rows(self, records):
        """records (window, head, threshold index, fired, score) -> feed()'s rows [keyword, time_ms, score, threshold]."""
        return [[self.keywords[n] if fired else input_data.SILENCE_LABEL, live_window_time_ms(w, self.hop_samples, self.sample_rate), score,
                 self.thresholds[k]] for w, n, k, fired, score in records]

    def _reset_detector(self, row):
        """Zeroes the detector state that belongs to row `row` of the frontend's."""
        self.dstates[row].zero_()

    def _reset_rows(self, row=None):
        """A new stream in `row` (None: in every row): its state slices zeroed, the host's mirror of its position too."""
        if row is None:
            self.fstates.zero_()
            self.dstates.zero_()
            self.spec.zero_()                           # (rows no push has written yet ride along in the embedding batch: the same after every reset)
            self.samples_pushed = [0] * self.streams    # the host's mirror of each state slice's first int64
        else:
            self.fstates[row].zero_()
            self._reset_detector(row)
            self.samples_pushed[row] = 0
        if hasattr(self, "resampler"):
            (self.rstates if row is None else self.rstates[row]).zero_()

    def _samples_seen(self, row, pending):
        return self.samples_pushed[row] // self.push_samples * self.in_push_samples + pending

    def _windows_seen(self, row):
        return live_windows(self.samples_pushed[row], self.window_samples, self.hop_samples)

    def close(self):
        self.graph = None
        self.probs = self.d_in = self.audio = self.active = self.fstates = self.dstates = self.spec = self.meta = self.out = None
        if hasattr(self, "resampler"):
            self.raw = self.rstates = None


class LiveSession(_LiveChain):
    """A live keyword spotter: fed audio chunks of any length, returns the detections those chunks completed.

    Where StreamingSession leaves the audio ring, 48 of every window's 49 frames and the detector to the caller, this session keeps the
    frontend's per-frame results and the detector's state in device memory between calls (include/mkws.h: mkws_frontend_live_push_f32,
    mkws_detect_live_step).  One push -- hops_per_push hops of NEW audio -- is one chain on one stream,
        frontend push (2 launches) -> mkws_embed_forward -> mkws_heads_forward -> detector step (1 launch),
    replayed as one hipGraph; per push the host uploads the new samples only and reads back one small buffer of counts and events.
    Every piece is bit-equal to its offline form: a push's spectrogram rows to Frontend.stream, its probabilities to
    StreamingSession.infer on that window (same launches on the same handle), its events to detect_on_device over the stream so far.
    The device side is _LiveChain's with one row (mkws_frontend_live_push_many_f32 and mkws_detect_live_step_many with n_streams = 1 and
    no mask: the launches of the one-stream calls): .fstate, .dstate and .rstate are row 0 of its state tensors, .meta is [1, 2 + h].

    models: TransferLearnedModel(s) sharing one embedding (or embedding= and heads=); keywords: their target words (default
    flags.target_keyword, or "keyword_<i>"); flags: a StreamFlags, of which average_window_duration_ms, suppression_ms, minimum_count,
    clip_duration_ms and clip_stride_ms are used; fired_only=False also reports the class's releases (label "_silence_").

    input_rate: the rate of the audio fed, when it is not the model's 16 kHz (None or 16000: the chain and the graph are exactly the
    ones above).  feed() then takes chunks at that rate, float32 or int16 PCM (which the cutter brings to float32 on the host, s / 32768: the
    upload is float32 either way); a push is live_in_samples(push_samples) of them, uploaded at their own rate, and the conversion (resample.Resampler.live_push_many, state in device memory like the other two) is the first launch of the
    chain.  samples_seen counts input-rate samples; windows and time_ms are in the 16 kHz timeline.  The live conversion is causal: its
    output lags the audio by Resampler.delay_ms (2 ms from 48 or 44.1 kHz, a tenth of a hop), which is not compensated.  A rate whose push
    is not a whole number of input samples raises ValueError naming the smallest hops_per_push that works (11 025 Hz: 2)."""

    def __init__(self, models=None, thresholds=(0.9,), flags=None, model_settings=None, hops_per_push=1, embedding=None, heads=None,
                 keywords=None, fired_only=True, use_graph=True, input_rate=None):
        # one row and no mask: the launches of the one-stream calls.  The host side is the session's own: a cutter, no scheduler, no mask
        # to fill or upload per push (profiles/live_group.txt: what a one-slot group pays for over a session)
        super().__init__(models, 1, thresholds, flags, model_settings, hops_per_push, embedding, heads, keywords, fired_only, input_rate,
                         masked=False)
        self.cutter = LivePushCutter(self.in_push_samples, pcm16=hasattr(self, "resampler"))
        self._start(use_graph)
        self.reset()

    fstate = property(lambda self: self.fstates[0], doc="the frontend's state block: row 0 of the one-row state tensor")
    dstate = property(lambda self: self.dstates[0], doc="the detector's state block")
    rstate = property(lambda self: self.rstates[0], doc="the resampler's state block (with input_rate only)")

    def reset(self):
        """Starts a new stream: the state blocks zeroed, the unfinished push dropped."""
        self._reset_rows()
        self.cutter.reset()
        self.last_records = []

    @property
    def samples_seen(self):
        return self._samples_seen(0, int(self.cutter.rest.size))

    @property
    def windows_seen(self):
        return self._windows_seen(0)

    def _push(self, samples):
        """One push of in_push_samples new samples (numpy) -> records (window, head, threshold index, fired, score) of the events it completed."""
        self.h_audio[0] = samples
        self._roundtrip()
        first = self.windows_seen
        self.samples_pushed[0] += self.push_samples
        records = self._unpack({0: first}).get(0, [])
        records.sort(key=lambda r: r[:3])
        return records

    def feed(self, chunk):
        """chunk: float32 samples of any length (numpy, CPU tensor or CUDA tensor, which is brought to the host: the pushes are cut
        there) -> [[keyword, time_ms, score, threshold], ...] for the events the chunk completed, ordered by window, keyword and
        threshold.  time_ms is the start of the window, as detect() reports it.  The same events as records (window, head index,
        threshold index, fired, score) are kept in .last_records."""
        records = []
        for samples in self.cutter.cut(_fed_samples(chunk)):
            records.extend(self._push(samples))
        self.last_records = records
        return self._rows(records)


class LiveSessionGroup(_LiveChain):
    """`streams` live keyword spotters served in lockstep: slot s is fed chunks of any length and gets back the detections they completed,
    as from a LiveSession of its own, but a tick -- one push of every slot that has a whole push pending -- is ONE chain on one stream,
        frontend push of all slots (2 launches) -> mkws_embed_forward at batch streams * hops_per_push -> mkws_heads_forward
        -> detector step of all slots (1 launch),
    replayed as one hipGraph: per tick one pinned upload (the [S, push] audio and the active mask), one replay, one download of the packed
    counts and events, one synchronise.  The slots share the heads, thresholds and flags (LiveRoutedGroup below: keywords and thresholds per
    slot); their states are the rows of two device
    tensors (fstates, dstates: a row is a one-stream state block), and a slot that is not active in a tick is not touched by it.

    What is promised, piece by piece:
      * a slot's spectrogram rows are bit-equal to Frontend.stream over that slot's audio;
      * a tick's probabilities (.probs [N, S * h, 3], slot s in rows s * h ..) are torch.equal to the eager
        Head.forward_many(heads, embedding.forward(group.spec)) on the same handle;
      * a slot's events are byte-equal to detect_on_device over the probability rows that slot received;
      * LiveSessionGroup(streams=1, hops_per_push=h) returns exactly what LiveSession(hops_per_push=h) returns on the same handle (the
        embedding batch is the same and so is the plan).
    NOT promised: equality of a slot's probabilities with those of its own batch-1 LiveSession -- the embedding handle picks another plan
    at another batch size (equal up to its rounding; tools/bench_live_group.py measures the difference).

    Arguments as LiveSession's; streams * hops_per_push must not exceed the embedding handle's max_batch.  input_rate as LiveSession's:
    every slot is fed at that rate, the tick's one upload carries the unconverted samples [S, in_push] (float32) and the active mask, and the conversion of
    all slots is one more launch at the head of the chain (an inactive slot's resampler state is not touched either); samples_seen counts
    input-rate samples, and the causal delay of Resampler.delay_ms is not compensated."""

    def __init__(self, models=None, streams=1, thresholds=(0.9,), flags=None, model_settings=None, hops_per_push=1, embedding=None, heads=None,
                 keywords=None, fired_only=True, use_graph=True, input_rate=None):
        super().__init__(models, streams, thresholds, flags, model_settings, hops_per_push, embedding, heads, keywords, fired_only, input_rate,
                         masked=True)
        self._serve(use_graph)

    def _serve(self, use_graph):
        """The end of a group's constructor, its buffers made: the scheduler, the first run and the capture, every slot at its start."""
        self.scheduler = LiveGroupScheduler(self.streams, self.in_push_samples, pcm16=hasattr(self, "resampler"))
        self._start(use_graph)
        self.reset()

    def reset(self, slot=None):
        """Starts a new stream in `slot` (None: in every slot): its state slices zeroed, its unfinished push dropped."""
        slot = None if slot is None else self.scheduler.slot(slot)
        self._reset_rows(slot)
        self.scheduler.reset(slot)
        self.last_records = {}

    def samples_seen(self, slot):
        return self._samples_seen(self.scheduler.slot(slot), self.scheduler.pending(slot))

    def windows_seen(self, slot):
        return self._windows_seen(self.scheduler.slot(slot))

    def _exchange(self, active, audio):
        """The device part of one tick (LiveGroupScheduler's) and the host mirrors of the slots' positions advanced.  -> {active slot:
        index of its first new window}."""
        self.h_audio[:] = audio
        self.h_active[:] = active
        self._roundtrip()
        on = np.flatnonzero(active).tolist()
        first = {s: self._windows_seen(s) for s in on}
        for s in on:
            self.samples_pushed[s] += self.push_samples
        return first

    def _tick(self, active, audio, records):
        """One tick: appends the records of the events it completed (_unpack's, ordered by window, head or route, threshold) to records[slot]."""
        for s, rec in self._unpack(self._exchange(active, audio)).items():
            rec.sort(key=lambda r: r[:3])
            records.setdefault(s, []).extend(rec)

    def feed(self, chunks):
        """chunks: {slot: samples} or a length-S sequence with None for silent slots; samples are float32 of any length (numpy, CPU or CUDA
        tensor, which is brought to the host: the pushes are cut there).  Runs the ticks the chunks complete -> {slot: [[keyword, time_ms,
        score, threshold], ...]} with one entry per slot fed, each slot's rows ordered as LiveSession.feed orders them.  The same events
        as records (window, head index, threshold index, fired, score) are kept per slot in .last_records."""
        fed = [(k, _fed_samples(v)) for k, v in self.scheduler.chunks(chunks)]
        records = {k: [] for k, _ in fed}
        for active, audio in self.scheduler.feed(dict(fed)):
            self._tick(active, audio, records)
        self.last_records = records
        return {k: self._rows(rec) for k, rec in records.items()}


class LiveRouteTable:
    """The host mirror of a route table: `max_routes` routes over `streams` slots and `n_heads` entries of a head table, `n_thresholds`
    thresholds each.  route_slot int32 [R] (-1: free), route_head int32 [R], thresholds float64 [R, T] are what the device copies hold
    after the next upload; .dirty says that they differ from them.  No device work: attach and detach only edit the mirrors."""

    def __init__(self, streams, n_heads, max_routes, n_thresholds, average_window_duration_ms=0):
        self.streams, self.n_heads, self.max_routes, self.n_thresholds = int(streams), int(n_heads), int(max_routes), int(n_thresholds)
        if self.streams < 1 or self.n_heads < 1 or self.max_routes < 1 or not 1 <= self.n_thresholds <= 1024:
            raise ValueError(f"LiveRouteTable({streams}, {n_heads}, {max_routes}, {n_thresholds}): at least one slot, head and route, 1 .. 1024 thresholds")
        self.avg = average_window_duration_ms
        self.route_slot = np.full(self.max_routes, -1, np.int32)
        self.route_head = np.zeros(self.max_routes, np.int32)
        self.thresholds = np.zeros((self.max_routes, self.n_thresholds), np.float64)
        self.keywords = [None] * self.max_routes
        self.dirty = True                                # nothing has been uploaded yet

    def route(self, route):
        if not 0 <= int(route) < self.max_routes:
            raise ValueError(f"route {route}: from 0 to {self.max_routes - 1}")
        return int(route)

    def attach(self, slot, head_index, keyword, thresholds):
        """-> the route id: the lowest free one.  ValueError for a full table, a slot or head index out of range, and anything but
        n_thresholds thresholds."""
        from ..detector import _check_thresholds
        thr = _check_thresholds(thresholds, self.avg)
        if thr.size != self.n_thresholds:
            raise ValueError(f"{thr.size} thresholds for a table of {self.n_thresholds} per route")
        if not 0 <= int(slot) < self.streams:
            raise ValueError(f"slot {slot}: from 0 to {self.streams - 1}")
        if not 0 <= int(head_index) < self.n_heads:
            raise ValueError(f"head index {head_index}: from 0 to {self.n_heads - 1}")
        free = np.flatnonzero(self.route_slot < 0)
        if free.size == 0:
            raise ValueError(f"the route table is full ({self.max_routes} routes)")
        r = int(free[0])
        self.route_slot[r], self.route_head[r], self.thresholds[r], self.keywords[r] = int(slot), int(head_index), thr, str(keyword)
        self.dirty = True
        return r

    def detach(self, route):
        r = self.route(route)
        if self.route_slot[r] >= 0:
            self.route_slot[r], self.keywords[r] = -1, None
            self.dirty = True

    def routes_of(self, slot):
        return np.flatnonzero(self.route_slot == int(slot)).tolist()

    def words(self):
        """The three tables as the int64 words of one upload (_lib.pack_words): route_slot | route_head | thresholds."""
        from .._lib import pack_words
        return pack_words([self.route_slot, self.route_head, self.thresholds])


class LiveRoutedGroup(LiveSessionGroup):
    """LiveSessionGroup whose slots each spot their own keywords: a ROUTE says "this slot listens for this entry of the head table at
    these thresholds", and heads and detectors do work per route instead of per (slot, head).  A tick is ONE chain on one stream,
        frontend push of all slots (2 launches) -> mkws_embed_forward at batch streams * hops_per_push
        -> mkws_head_group_forward_routes -> mkws_detect_live_step_routes,
    replayed as one hipGraph: per tick one pinned upload (audio and active mask), one replay, one download of max_routes * n_thresholds
    counts and their events, one synchronise.  The route table (route_slot, route_head, thresholds) lives in device memory and is read by
    the kernels: attach() and detach() edit host mirrors and set .table.dirty, the next tick uploads the three small tables before its
    replay, ordered on the same stream.  Nothing is re-captured: .graph stays the same object and .recaptures stays 0.

    heads: a list of Head objects of equal dimensions, held in one HeadGroup created once; entries no route names are spare.
    Head.set_params on an entry is how a newly fine-tuned keyword enters the table (the group holds device pointers).

    What is promised, piece by piece:
      * the frontend and embedding legs are LiveSessionGroup's, unchanged;
      * a tick's probabilities (.probs [max_routes, h, 3]) are, for every attached route, torch.equal to Head.forward of its head on its
        slot's rows of embedding.forward(group.spec);
      * a route's events are byte-equal to detect_on_device over the probability rows it received since attach(), at its slot's window
        times, with its own thresholds: a route attached in mid-stream starts with a fresh detector;
      * with every slot routed to every head at the same thresholds, feed() returns LiveSessionGroup's rows, scores bit-equal; within a
        window the rows are ordered by route id, then threshold."""

    def __init__(self, embedding, heads, streams, max_routes, n_thresholds=1, flags=None, model_settings=None, hops_per_push=1, fired_only=True,
                 use_graph=True, input_rate=None):
        import torch
        self._resolve(None, embedding, heads, streams, hops_per_push)
        if not self.heads:
            raise ValueError("LiveRoutedGroup: at least one head in the table")
        self.flags = flags if flags is not None else default_live_flags([])
        self.table = LiveRouteTable(self.streams, len(self.heads), max_routes, n_thresholds, self.flags.average_window_duration_ms)
        ms = self._geometry(model_settings, fired_only)
        self._input(input_rate)
        dev = embedding.device
        R, T, h = self.table.max_routes, self.table.n_thresholds, self.hops
        with torch.cuda.device(dev):
            self.head_group = HeadGroup(self.heads)
            self._slot_buffers(ms)
            self.dstates = live_detector_state_routes(R, T, self.history, device=dev)
            # the route table, ONE buffer so that an edit is one upload: route_slot [R] | route_head [R] (int32) | thresholds [R, T] (float64)
            words, offsets = self.table.words()
            self.d_table = torch.zeros(words.size, dtype=torch.int64, device=dev)
            self.h_table = torch.zeros(words.size, dtype=torch.int64).pin_memory()
            as_bytes = self.d_table.view(torch.uint8)
            self.route_slot = as_bytes[offsets[0]:offsets[0] + 4 * R].view(torch.int32)
            self.route_head = as_bytes[offsets[1]:offsets[1] + 4 * R].view(torch.int32)
            self.d_thr = as_bytes[offsets[2]:offsets[2] + 8 * R * T].view(torch.float64).view(R, T)
            self.probs_buf = torch.zeros((R, h, self.heads[0].classes), dtype=torch.float32, device=dev)
            self.invalid = torch.zeros(1, dtype=torch.int32, device=dev)
            self._out_buffers(live_out_words_routes(R, T, h))
            self._before_replay()                        # the empty table: every route disabled
        self._serve(use_graph)
        torch.cuda.current_stream(dev).synchronize()     # (the pinned mirror of the table is free to be edited)

    def attach(self, slot, head_index, keyword, thresholds):
        """Slot `slot` listens for entry `head_index` of the head table, reported as `keyword`, at these n_thresholds thresholds -> the
        route id (the lowest free one).  The route starts with a fresh detector at the next tick.  Host work and one small memset; nothing
        is re-captured."""
        r = self.table.attach(slot, head_index, keyword, thresholds)
        self.dstates[r].zero_()
        return r

    def detach(self, route):
        """Disables the route: from the next tick on it is neither computed nor reported."""
        self.table.detach(route)

    def _before_replay(self):
        if self.table.dirty:
            self.h_table.numpy()[:] = self.table.words()[0]
            self.d_table.copy_(self.h_table, non_blocking=True)
            # what this tick's events are reported with (the host mirrors may be edited again before the next one)
            self._live = (self.table.route_slot.copy(), list(self.table.keywords), self.table.thresholds.copy())
            self.table.dirty = False

    def _chain(self):
        f = self.flags
        self._frontend_push()
        probs, _ = self.head_group.forward_routes(self.embedding.forward(self.spec), self.route_slot, self.route_head, self.hops, self.streams,
                                                  out=self.probs_buf, invalid=self.invalid)
        detect_live_step_routes(self.dstates, probs, self.meta, self.route_slot, self.d_thr, f.average_window_duration_ms, f.suppression_ms,
                                f.minimum_count, self.history, target_id=2, fired_only=self.fired_only, out=self.out)
        return probs

    def _reset_detector(self, row):
        """The detector slices of a slot are those of the routes attached to it."""
        for r in self.table.routes_of(row):
            self.dstates[r].zero_()

    def close(self):
        super().close()
        self.d_table = self.route_slot = self.route_head = self.d_thr = self.probs_buf = self.invalid = None
        if getattr(self, "head_group", None) is not None:
            self.head_group.close()
            self.head_group = None

    def _unpack(self, first):
        """-> {slot: records (window, route, threshold index, fired, score, keyword, threshold)}, with the table as this tick ran it."""
        slots, keywords, thresholds = self._live
        counts, events = live_unpack_many(self.h_out.numpy(), self.table.max_routes, 1, self.table.n_thresholds, self.hops)
        fresh = {}
        if counts.any():
            for r, _, k in zip(*np.nonzero(counts)):
                s = int(slots[r])
                for w, fired, score in events[r, 0, k, :counts[r, 0, k]].tolist():
                    fresh.setdefault(s, []).append((first[s] + w, int(r), int(k), fired, score, keywords[r], float(thresholds[r, k])))
        return fresh

    def _rows(self, records):
        return [[kw if fired else input_data.SILENCE_LABEL, live_window_time_ms(w, self.hop_samples, self.sample_rate), score, thr]
                for w, _, _, fired, score, kw, thr in records]

