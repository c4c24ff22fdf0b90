"""Sample-rate conversion on the device: thin host wrapper over mkws_resample_* (include/mkws.h).

A rational-ratio polyphase FIR resampler with a stated filter (Kaiser-windowed sinc, computed in double on the host).  Two forms: the
stateless batch form for clips and whole recordings (Resampler.forward, centred = time-aligned by default) and the live form whose
per-stream state lives in a device block of the caller's (Resampler.live_push_many: causal, delayed by Resampler.delay_ms).  The host
helpers geometry / host_taps / out_samples work without a GPU, as frontend.host_table does."""
import ctypes

import numpy as np

from . import _lib


def make_cfg(rate_in, rate_out=16000, **over):
    cfg = _lib.ResampleCfg()
    _lib.lib().mkws_resample_default_cfg(ctypes.byref(cfg), int(rate_in), int(rate_out))
    for k, v in over.items():
        if k in ("rate_in", "rate_out") or not hasattr(cfg, k):
            raise TypeError(f"unknown resampler option {k!r}")
        setattr(cfg, k, int(v) if isinstance(getattr(cfg, k), int) else float(v))
    return cfg


def geometry(cfg):
    """Host-only: {L, M, T, half} of include/mkws.h's definitions (MkwsError for a configuration the library refuses)."""
    out = (ctypes.c_int32 * 4)()
    _lib.check(_lib.lib().mkws_resample_geometry(ctypes.byref(cfg), out))
    return dict(zip(("L", "M", "T", "half"), (int(v) for v in out)))


def host_taps(cfg):
    """Host-only: the table tab[j * L + p] as float32 [T, L]."""
    L = _lib.lib()
    g = geometry(cfg)
    n = _lib.check(L.mkws_resample_host_taps(ctypes.byref(cfg), None, 0))
    buf = np.zeros(n, dtype=np.float32)
    _lib.check(L.mkws_resample_host_taps(ctypes.byref(cfg), buf.ctypes.data, n))
    return buf.reshape(g["T"], g["L"])


def out_samples(cfg, n_in):
    """Host-only: ceil(n_in * L / M)."""
    return int(_lib.check(_lib.lib().mkws_resample_out_samples(ctypes.byref(cfg), int(n_in))))


def live_in_samples(cfg, n_out):
    """Host-only: input samples of a live push of n_out output samples, n_out * M / L; ValueError when that is not a whole number
    (what mkws_resample_live_in_samples refuses)."""
    g = geometry(cfg)
    if int(n_out) < 0 or (int(n_out) * g["M"]) % g["L"]:
        raise ValueError(f"a push of {n_out} output samples is {int(n_out) * g['M']}/{g['L']} input samples at {cfg.rate_in} -> {cfg.rate_out} Hz, "
                         "not a whole number")
    return int(n_out) * g["M"] // g["L"]


def live_push_hops(rate_in, rate_out, hop_samples):
    """The smallest hops_per_push whose push of hops * hop_samples output samples is a whole number of input samples."""
    g = int(np.gcd(int(rate_in), int(rate_out)))
    L, M = int(rate_out) // g, int(rate_in) // g
    return L // int(np.gcd(int(hop_samples) * M, L))


class Resampler:
    """One configured device resampler rate_in -> rate_out (the table uploaded once).  Options: zero_crossings (32), kaiser_beta (9.0),
    rolloff (0.95)."""

    def __init__(self, rate_in, rate_out=16000, **cfg):
        self.cfg = make_cfg(rate_in, rate_out, **cfg)
        self.rate_in, self.rate_out = int(rate_in), int(rate_out)
        self.geometry = geometry(self.cfg)
        self.L = _lib.lib()
        h = ctypes.c_void_p()
        _lib.check(self.L.mkws_resample_create(ctypes.byref(self.cfg), ctypes.byref(h)))
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            self.L.mkws_resample_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def taps(self):
        return host_taps(self.cfg)

    def out_samples(self, n):
        return out_samples(self.cfg, n)

    @property
    def delay_ms(self):
        """The delay of the causal form against the centred one: half / (L * rate_in) seconds = zero_crossings / min(rates)."""
        return 1000.0 * self.geometry["half"] / (self.geometry["L"] * self.rate_in)

    def forward(self, audio, centred=True, out=None):
        """audio: numpy array or tensor, [n] or [B, n], float32 or int16 PCM -> float32 of the same kind and rank with out_samples(n)
        samples per row.  A CUDA tensor stays on its device (rows may be strided; asynchronous on the current stream); anything else is
        uploaded and the result comes back to the host."""
        import torch
        is_np = not torch.is_tensor(audio)
        a = torch.from_numpy(np.ascontiguousarray(audio)) if is_np else audio
        if a.dtype not in (torch.float32, torch.int16):
            raise TypeError(f"audio must be float32 or int16, got {a.dtype}")
        if a.dim() not in (1, 2):
            raise ValueError("audio must be [n] or [B, n]")
        host = not a.is_cuda
        d = a.cuda() if host else a
        rows = d[None] if d.dim() == 1 else d
        if rows.shape[1] > 1 and rows.stride(1) != 1 or (rows.shape[0] > 1 and rows.stride(0) < rows.shape[1]):
            rows = rows.contiguous()
        B, n = rows.shape
        n_out = self.out_samples(n)
        if out is None:
            out = torch.empty((B, n_out), dtype=torch.float32, device=rows.device)
        elif not out.is_cuda or out.device != rows.device or out.dtype != torch.float32 or tuple(out.shape) != (B, n_out) or (n_out > 1 and out.stride(1) != 1) \
                or (B > 1 and out.stride(0) < n_out):
            raise ValueError(f"out must be a CUDA float32 tensor [{B}, {n_out}] with contiguous rows that do not overlap, on the device of audio")
        if B and n:
            with torch.cuda.device(rows.device):
                _lib.check(self.L.mkws_resample_forward(
                    self.h, ctypes.c_void_p(rows.data_ptr()), int(rows.dtype == torch.int16), B, n, int(rows.stride(0)) if B > 1 else n,
                    int(bool(centred)), ctypes.c_void_p(out.data_ptr()), int(out.stride(0)) if B > 1 else n_out, _lib.current_stream_ptr()))
        res = out[0] if a.dim() == 1 else out
        if host:
            res = res.cpu()
        return res.numpy() if is_np else res

    # -- live form (mkws_resample_live_push_many): causal, the state in a device block of the caller's ------------------------------------
    def live_in_samples(self, out_samples):
        """Input samples of a push of out_samples output samples; ValueError when that is not a whole number."""
        n = self.L.mkws_resample_live_in_samples(self.h, int(out_samples))
        if n < 0:
            raise ValueError(self.L.mkws_last_error().decode("utf-8", "replace"))
        return n

    def live_state_many(self, streams, device=None):
        """Zero-filled state blocks of `streams` fresh streams: an int64 CUDA tensor [streams, words]; row s is a one-stream block
        (.zero_() resets it, .clone() / .copy_() snapshot and restore it).  Its first element is the number of input samples pushed."""
        import torch
        if int(streams) < 0:
            raise ValueError(f"live_state_many: {streams} streams")
        words = self.L.mkws_resample_live_state_bytes(self.h) // 8
        return torch.zeros((int(streams), words), dtype=torch.int64, device=device if device is not None else "cuda")

    def live_push_many(self, states, audio, out_samples, active=None, out=None):
        """One push of every active stream.  states: live_state_many(S); audio: contiguous CUDA float32 or int16
        [S, live_in_samples(out_samples)], the NEW samples of each stream; active: CUDA int32 [S] (None = all) -> out float32
        [S, out_samples], the next out_samples causal output samples of each active stream (the rows of the others are untouched).
        Asynchronous, allocation-free when out is passed in, one launch for any S."""
        import torch
        from .frontend import check_live_many, check_live_many_tensors
        n_in = self.live_in_samples(out_samples)
        check_live_many(states, audio.shape if audio.dim() == 2 else None, n_in, "audio")
        S = int(states.shape[0])
        if not audio.is_cuda or audio.dtype not in (torch.float32, torch.int16) or not audio.is_contiguous():
            raise ValueError(f"live_push_many takes a contiguous CUDA float32 or int16 tensor [{S}, {n_in}] of new samples")
        if active is not None and (not active.is_cuda or active.dtype != torch.int32 or not active.is_contiguous() or active.numel() != S):
            raise ValueError(f"active must be a contiguous CUDA int32 tensor [{S}]")
        if out is not None and (not out.is_cuda or out.dtype != torch.float32 or out.numel() != S * int(out_samples) or not out.is_contiguous()):
            raise ValueError(f"out must be a contiguous CUDA float32 tensor of {S} x {int(out_samples)} samples")
        check_live_many_tensors("live_push_many", audio.device, states=(states, torch.int64), active=(active, torch.int32), out=(out, torch.float32))
        if out is None:                        # (nothing is allocated before everything the caller gave has been accepted)
            out = torch.zeros((S, int(out_samples)), dtype=torch.float32, device=audio.device)
        with torch.cuda.device(audio.device):
            _lib.check(self.L.mkws_resample_live_push_many(
                self.h, ctypes.c_void_p(states.data_ptr()), 8 * int(states.stride(0)), S,
                ctypes.c_void_p(active.data_ptr()) if active is not None else None, ctypes.c_void_p(audio.data_ptr()),
                int(audio.dtype == torch.int16), int(out_samples), ctypes.c_void_p(out.data_ptr()), _lib.current_stream_ptr()))
        return out
