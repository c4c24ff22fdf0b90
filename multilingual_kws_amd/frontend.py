"""Device micro-frontend handle: thin host wrapper over mkws_frontend_* (include/mkws.h)."""
import ctypes

import numpy as np

from . import _lib

_TABLE_IDS = dict(window_coef=(0, np.int16), twiddles=(1, np.int16), super_twiddles=(2, np.int16),
                  weights=(3, np.int16), unweights=(4, np.int16), chan_freq_starts=(5, np.int16),
                  chan_weight_starts=(6, np.int16), chan_widths=(7, np.int16), gain_lut=(8, np.int16),
                  log_lut=(9, np.uint16), scalars=(10, np.int32))
_SCALARS = ("window_size", "window_step", "fft_size", "start_index", "end_index", "num_weights",
            "snr_shift", "correction_bits")


def make_cfg(**over):
    cfg = _lib.FrontendCfg()
    _lib.lib().mkws_frontend_default_cfg(ctypes.byref(cfg))
    for k, v in over.items():
        if not hasattr(cfg, k):
            raise TypeError(f"unknown frontend option {k!r}")
        setattr(cfg, k, int(v) if isinstance(getattr(cfg, k), int) else float(v))
    return cfg


def host_table(cfg, name):
    """Host-only (works without a GPU): one of the integer tables the library builds for cfg."""
    which, dt = _TABLE_IDS[name]
    L = _lib.lib()
    n = _lib.check(L.mkws_frontend_host_table(ctypes.byref(cfg), which, None, 0))
    buf = np.zeros(n // np.dtype(dt).itemsize, dtype=dt)
    _lib.check(L.mkws_frontend_host_table(ctypes.byref(cfg), which, buf.ctypes.data, n))
    return buf


def host_scalars(cfg):
    return dict(zip(_SCALARS, host_table(cfg, "scalars").tolist()))


def num_frames(cfg, n_samples):
    return _lib.check(_lib.lib().mkws_frontend_num_frames(ctypes.byref(cfg), n_samples))


class Frontend:
    """One configured device frontend (tables uploaded once).  All tensors are torch CUDA tensors."""

    def __init__(self, max_samples=16000, **cfg_over):
        self.cfg = make_cfg(**cfg_over)
        self.L = _lib.lib()
        h = ctypes.c_void_p()
        _lib.check(self.L.mkws_frontend_create(ctypes.byref(self.cfg), int(max_samples), ctypes.byref(h)))
        self.h = h
        self.max_samples = int(max_samples)
        self.num_channels = self.cfg.num_channels

    def close(self):
        if getattr(self, "h", None):
            self.L.mkws_frontend_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def forward(self, audio, want_raw=False, out=None):
        """audio: CUDA tensor [B, n] float32 in [-1,1] or int16 PCM -> float32 [B, frames, channels]
        (= to_micro_spectrogram); with want_raw also the op's raw integers (int16 storage of uint16)."""
        import torch
        if not torch.is_tensor(audio) or not audio.is_cuda:
            raise ValueError("Frontend.forward needs a CUDA tensor (no CPU path)")
        B, n, F = check_forward(self.cfg, audio.device, audio, out)
        if audio.dim() == 1:
            audio = audio[None]
        audio = audio.contiguous()
        spec = out if out is not None else torch.empty((B, F, self.num_channels), dtype=torch.float32, device=audio.device)
        raw = torch.empty((B, F, self.num_channels), dtype=torch.int16, device=audio.device) if want_raw else None
        rp = ctypes.c_void_p(raw.data_ptr()) if want_raw else None
        if B == 0 or F == 0:                  # empty in -> empty out, like the op
            return (spec, raw) if want_raw else spec
        if audio.dtype == torch.float32:
            fn = self.L.mkws_frontend_forward_f32
        elif audio.dtype == torch.int16:
            fn = self.L.mkws_frontend_forward_i16
        else:
            raise TypeError(f"audio must be float32 or int16, got {audio.dtype}")
        with torch.cuda.device(audio.device):
            _lib.check(fn(self.h, ctypes.c_void_p(audio.data_ptr()), B, n, ctypes.c_void_p(spec.data_ptr()), rp,
                          _lib.current_stream_ptr()))
        return (spec, raw) if want_raw else spec

    def stream(self, audio, window_samples, hop_samples, want_raw=False):
        """One long recording [n] float32 -> [num_windows, frames, channels], window w covering
        samples [w*hop, w*hop+window) -- batch_streaming_analysis.py:99-117 with frame sharing."""
        import torch
        if not torch.is_tensor(audio) or not audio.is_cuda:
            raise ValueError("Frontend.stream: audio must be a CUDA tensor (no CPU path)")
        n, F, nw = check_stream(self.cfg, audio.device, audio, window_samples, hop_samples)
        audio = audio.contiguous()
        spec = torch.empty((nw, F, self.num_channels), dtype=torch.float32, device=audio.device)
        raw = torch.empty((nw, F, self.num_channels), dtype=torch.int16, device=audio.device) if want_raw else None
        if nw > 0:
            with torch.cuda.device(audio.device):
                got = _lib.check(self.L.mkws_frontend_stream_f32(
                    self.h, ctypes.c_void_p(audio.data_ptr()), n, window_samples, hop_samples,
                    ctypes.c_void_p(spec.data_ptr()), ctypes.c_void_p(raw.data_ptr()) if want_raw else None,
                    nw, _lib.current_stream_ptr()))
            assert got == nw
        return (spec, raw) if want_raw else spec

    # -- live form (mkws_frontend_live_push_f32): the stream fed push by push, its state in a device block of the caller's ------------
    def live_state(self, window_samples, hop_samples, hops_per_push=1, device=None):
        """A zero-filled state block (int64 CUDA tensor) = a fresh stream of pushes of hops_per_push * hop_samples samples.  Reset is
        .zero_(), snapshot .clone(), restore .copy_(); its first element is the number of samples pushed so far.  ValueError for a geometry
        the push refuses (a hop that is not a multiple of the frame step, ...)."""
        import torch
        n = self.L.mkws_frontend_live_state_bytes(self.h, int(window_samples), int(hop_samples), int(hops_per_push))
        if n == 0:                 # (a size carries no status: what the push would refuse, in the library's own words)
            raise ValueError("no live frontend state: " + self.L.mkws_last_error().decode("utf-8", "replace"))
        return torch.zeros((n + 7) // 8, dtype=torch.int64, device=device if device is not None else "cuda")

    def live_push(self, state, audio, window_samples, hop_samples, hops_per_push=1, spec=None, raw=None, meta=None, want_raw=False):
        """One push: audio CUDA float32 [hops_per_push * hop_samples], the NEW samples -> (spec float32 [hops_per_push, frames, channels],
        raw, meta int64 [2 + hops_per_push] = {count, index of the first new window, time_ms of each}); raw holds the op's raw integers
        with want_raw (or raw=) and is None otherwise.  Rows 0 .. count-1 hold the windows the push completed, bit-equal to the same rows of stream() over
        the whole recording; the others are left as they were.  Asynchronous, allocation-free when spec / raw / meta are passed in
        (static buffers of a captured graph), and the state advances on the device: a replay is a push."""
        import torch
        h = int(hops_per_push)
        if not torch.is_tensor(audio) or not audio.is_cuda:
            raise ValueError(f"live_push: audio must be a contiguous CUDA float32 tensor of {h} x {int(hop_samples)} new samples")
        # (a size of 0 = a geometry the push refuses: the C call says why, before it looks at a buffer)
        need = self.L.mkws_frontend_live_state_bytes(self.h, int(window_samples), int(hop_samples), h)
        F = check_live_push(self.cfg, audio.device, need, state, audio, window_samples, hop_samples, h, spec, raw, meta)
        if spec is None:
            spec = torch.zeros((h, F, self.num_channels), dtype=torch.float32, device=audio.device)
        if raw is None and want_raw:
            raw = torch.zeros((h, F, self.num_channels), dtype=torch.int16, device=audio.device)
        if meta is None:
            meta = torch.zeros(2 + h, dtype=torch.int64, device=audio.device)
        with torch.cuda.device(audio.device):
            _lib.check(self.L.mkws_frontend_live_push_f32(
                self.h, ctypes.c_void_p(state.data_ptr()), ctypes.c_void_p(audio.data_ptr()), int(window_samples), int(hop_samples), h,
                ctypes.c_void_p(spec.data_ptr()), ctypes.c_void_p(raw.data_ptr()) if raw is not None else None,
                ctypes.c_void_p(meta.data_ptr()), _lib.current_stream_ptr()))
        return spec, raw, meta

    # -- many live streams in lockstep (mkws_frontend_live_push_many_f32): one push for all of them, two launches for any number -------
    def live_state_many(self, streams, window_samples, hop_samples, hops_per_push=1, device=None):
        """Zero-filled state blocks of `streams` fresh streams: an int64 CUDA tensor [streams, words] whose row stride is the state
        stride, so row s viewed flat is a valid one-stream state (live_push takes it, .zero_() resets that stream alone)."""
        import torch
        if int(streams) < 0:
            raise ValueError(f"live_state_many: {streams} streams")
        words = self.live_state(window_samples, hop_samples, hops_per_push, device=device).numel()
        return torch.zeros((int(streams), words), dtype=torch.int64, device=device if device is not None else "cuda")

    def live_push_many(self, states, audio, window_samples, hop_samples, hops_per_push=1, active=None, spec=None, raw=None, meta=None,
                       want_raw=False):
        """One push of every active stream.  states: live_state_many(S, ...); audio CUDA float32 [S, hops_per_push * hop_samples], the
        NEW samples of each stream; active: CUDA int32 [S] (None = all) -> (spec float32 [S * hops_per_push, frames, channels], raw,
        meta int64 [S, 2 + hops_per_push]).  Stream s owns rows s * hops_per_push .. + meta[s, 0] - 1 of spec / raw -- the layout of one
        embedding batch -- and what it gets is live_push on its own slice, bit for bit.  A stream with active[s] == 0 is not advanced:
        its state and rows are untouched and its meta row says count = 0.  Asynchronous, allocation-free when spec / raw / meta are
        passed in, two launches for any S."""
        import torch
        h = int(hops_per_push)
        check_live_many(states, audio.shape if audio.dim() == 2 else None, h * int(hop_samples), "audio")
        S = int(states.shape[0])
        if not audio.is_cuda or audio.dtype != torch.float32 or not audio.is_contiguous():
            raise ValueError(f"live_push_many takes a contiguous CUDA float32 tensor [{S}, {h} x {int(hop_samples)}] of new samples")
        if active is not None and (not active.is_cuda or active.dtype != torch.int32 or not active.is_contiguous() or active.numel() != S):
            raise ValueError(f"active must be a contiguous CUDA int32 tensor [{S}]")
        F = num_frames(self.cfg, window_samples)
        for name, t, n in (("spec", spec, S * h * F * self.num_channels), ("raw", raw, S * h * F * self.num_channels), ("meta", meta, S * (2 + h))):
            if t is not None and (t.numel() != n or not t.is_contiguous()):
                raise ValueError(f"{name} must be contiguous with {n} elements")
        check_live_many_tensors("live_push_many", audio.device, states=(states, torch.int64), active=(active, torch.int32), spec=(spec, torch.float32),
                                raw=(raw, torch.int16), meta=(meta, torch.int64))
        if spec is None:                       # (nothing is allocated before everything the caller gave has been accepted)
            spec = torch.zeros((S * h, F, self.num_channels), dtype=torch.float32, device=audio.device)
        if raw is None and want_raw:
            raw = torch.zeros((S * h, F, self.num_channels), dtype=torch.int16, device=audio.device)
        if meta is None:
            meta = torch.zeros((S, 2 + h), dtype=torch.int64, device=audio.device)
        with torch.cuda.device(audio.device):
            _lib.check(self.L.mkws_frontend_live_push_many_f32(
                self.h, ctypes.c_void_p(states.data_ptr()), 8 * int(states.stride(0)), S,
                ctypes.c_void_p(active.data_ptr()) if active is not None else None, ctypes.c_void_p(audio.data_ptr()),
                int(window_samples), int(hop_samples), h, ctypes.c_void_p(spec.data_ptr()),
                ctypes.c_void_p(raw.data_ptr()) if raw is not None else None, ctypes.c_void_p(meta.data_ptr()), _lib.current_stream_ptr()))
        return spec, raw, meta


def _describe(t):
    import torch
    return f"{t.dtype} {tuple(t.shape)} (strides {t.stride()}) on {t.device}" if torch.is_tensor(t) else type(t).__name__


def check_forward(cfg, device, audio, out=None):
    """What Frontend.forward refuses, decided before any device call: audio a float32 or int16 tensor [B, n] or [n] on `device` (a
    strided view is made contiguous by the wrapper; TypeError for another dtype); `out` (if given) a contiguous float32 tensor
    [rows >= B, frames, channels] on `device`.  -> (B, n, frames).  ValueError otherwise."""
    import torch
    if not torch.is_tensor(audio) or audio.dim() not in (1, 2) or audio.device != device:
        raise ValueError(f"Frontend.forward: audio must be a tensor [B, n] or [n] on {device}, got {_describe(audio)}")
    if audio.dtype not in (torch.float32, torch.int16):
        raise TypeError(f"audio must be float32 or int16, got {audio.dtype}")
    B, n = (1, int(audio.shape[0])) if audio.dim() == 1 else (int(audio.shape[0]), int(audio.shape[1]))
    F = num_frames(cfg, n)
    C = cfg.num_channels
    if out is not None and (not torch.is_tensor(out) or out.dim() != 3 or tuple(out.shape[1:]) != (F, C) or out.shape[0] < B or out.dtype != torch.float32
                            or not out.is_contiguous() or out.device != device):
        raise ValueError(f"Frontend.forward: out must be a contiguous float32 tensor [{B}, {F}, {C}] on {device}, got {_describe(out)}")
    return B, n, F


def check_stream(cfg, device, audio, window_samples, hop_samples):
    """What Frontend.stream refuses, decided before any device call: audio a float32 vector [n] on `device` (a strided view is made
    contiguous by the wrapper), a window and a hop of at least one sample.  -> (n, frames, num_windows).  ValueError otherwise."""
    import torch
    if not torch.is_tensor(audio) or audio.dim() != 1 or audio.dtype != torch.float32 or audio.device != device:
        raise ValueError(f"Frontend.stream: audio must be a float32 vector [n] on {device}, got {_describe(audio)}")
    if int(window_samples) < 1 or int(hop_samples) < 1:
        raise ValueError(f"Frontend.stream: window_samples={window_samples}, hop_samples={hop_samples}")
    n = int(audio.shape[0])
    return n, num_frames(cfg, int(window_samples)), live_windows(n, int(window_samples), int(hop_samples))


def check_live_push(cfg, device, state_bytes, state, audio, window_samples, hop_samples, hops_per_push, spec=None, raw=None, meta=None):
    """What Frontend.live_push refuses, decided before any device call.  state_bytes: mkws_frontend_live_state_bytes for this geometry (0: the
    geometry itself is refused by the C call, and the state's size is not judged here).  state a contiguous int64 tensor of at least
    state_bytes bytes; audio a contiguous float32 tensor of hops_per_push * hop_samples samples; spec (if given) contiguous float32 and raw
    (if given) contiguous int16 of at least hops_per_push * frames * channels elements; meta (if given) contiguous int64 of at least
    2 + hops_per_push elements; all on `device`.  -> frames.  ValueError otherwise."""
    import torch
    h = int(hops_per_push)
    if not torch.is_tensor(audio) or audio.dtype != torch.float32 or not audio.is_contiguous() or audio.numel() != h * int(hop_samples) or audio.device != device:
        raise ValueError(f"live_push: audio must be a contiguous float32 tensor of {h} x {int(hop_samples)} new samples on {device}, got {_describe(audio)}")
    if not torch.is_tensor(state) or state.dtype != torch.int64 or not state.is_contiguous() or 8 * state.numel() < int(state_bytes) or state.device != device:
        raise ValueError(f"live_push: state must be a contiguous int64 tensor of at least {(int(state_bytes) + 7) // 8} words on {device} (live_state), "
                         f"got {_describe(state)}")
    F = num_frames(cfg, int(window_samples))
    rows = h * F * cfg.num_channels
    for name, t, dtype, n in (("spec", spec, torch.float32, rows), ("raw", raw, torch.int16, rows), ("meta", meta, torch.int64, 2 + h)):
        if t is not None and (not torch.is_tensor(t) or t.dtype != dtype or not t.is_contiguous() or t.numel() < n or t.device != device):
            raise ValueError(f"live_push: {name} must be a contiguous {dtype} tensor of {n} elements on {device}, got {_describe(t)}")
    return F


def check_live_many(states, shape, row, what):
    """The rules of a many-stream call that are decided before any device call: states is an int64 tensor [S, words] with unit inner
    stride (its row stride is the state stride), and the per-stream input has the shape [S, row].  ValueError otherwise."""
    import torch
    if states.dim() != 2 or states.dtype != torch.int64 or (states.shape[1] > 1 and states.stride(1) != 1) or \
            (states.shape[0] > 1 and states.stride(0) < states.shape[1]):
        raise ValueError("states must be an int64 tensor [streams, words] whose rows are contiguous and do not overlap "
                         "(live_state_many / live_detector_state_many)")
    if shape is None or tuple(shape) != (int(states.shape[0]), int(row)):
        raise ValueError(f"{what} must have the shape [{int(states.shape[0])}, {int(row)}]: one row per stream of the state tensor")


def check_live_many_tensors(who, device, **tensors):
    """name=(tensor or None, dtype): what a many-stream call still has to refuse once shapes and strides are settled -- a tensor of another
    dtype, or one that does not live on `device` (the kernel would read it as `dtype` through a pointer of another device, or of the host).
    ValueError naming it."""
    for name, (t, dtype) in tensors.items():
        if t is not None and (t.dtype != dtype or t.device != device):
            raise ValueError(f"{who}: {name} must be a {dtype} tensor on {device}, got {t.dtype} on {t.device}")


def live_windows(n_samples, window_samples, hop_samples):
    """W(n): the windows that exist after n samples of a live stream (the num_windows of Frontend.stream)."""
    return 0 if n_samples < window_samples else 1 + (n_samples - window_samples) // hop_samples


def live_window_time_ms(w, hop_samples, sample_rate=16000):
    """Time of live window w, the start of the window: the int(offset * 1000 / sample_rate) of batch_streaming_analysis.detect()."""
    return (w * hop_samples * 1000) // sample_rate
