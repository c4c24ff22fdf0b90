"""Level normalisation on the device: thin host wrapper over mkws_loudness_* (include/mkws.h).

The BS.1770 integrated loudness (K-weighting, 400 ms blocks, the absolute and the relative gate), the 4x oversampled true peak, the sample
peak and the mean square of every row of a batch, and the linear gain that brings a row to target_lufs without its true peak passing
true_peak_db (mode "loudness"), or pydub's peak rule (mode "peak").  This is the measurement and the linear gain of loudnorm's two-pass
linear mode, not loudnorm's dynamic compressor.  make_cfg / coeffs / geometry work without a GPU."""
import ctypes

import numpy as np

from . import _lib

MODES = {"loudness": 0, "peak": 1}
FLAG_UNMEASURED, FLAG_PEAK_LIMITED = 1, 2
STATS = ("loudness", "true_peak", "sample_peak", "mean_square")
COUNTS = ("blocks", "absolute", "relative", "flags")


def make_cfg(rate=16000, **over):
    cfg = _lib.LoudnessCfg()
    _lib.lib().mkws_loudness_default_cfg(ctypes.byref(cfg), int(rate))
    for k, v in over.items():
        if k == "rate" or not hasattr(cfg, k):
            raise TypeError(f"unknown loudness option {k!r}")
        if k == "mode":
            if v not in MODES:
                raise ValueError(f"mode must be one of {sorted(MODES)}, got {v!r}")
            v = MODES[v]
        setattr(cfg, k, int(v) if isinstance(getattr(cfg, k), int) else float(v))
    return cfg


def coeffs(rate=16000):
    """Host-only: the K-weighting biquads at `rate` as float64 [2, 5]: rows shelf and high-pass, columns b0, b1, b2, a1, a2
    (MkwsError for a rate the library refuses)."""
    out = (ctypes.c_double * 10)()
    cfg = make_cfg(rate)
    _lib.check(_lib.lib().mkws_loudness_coeffs(ctypes.byref(cfg), out))
    return np.array(out, dtype=np.float64).reshape(2, 5)


def geometry(cfg):
    """Host-only: {hop, block, chunk, tile} of include/mkws.h's definitions."""
    out = (ctypes.c_int32 * 4)()
    _lib.check(_lib.lib().mkws_loudness_geometry(ctypes.byref(cfg), out))
    return dict(zip(("hop", "block", "chunk", "tile"), (int(v) for v in out)))


class LoudnessMeter:
    """One configured device meter at `rate` Hz with a workspace for max_rows rows of max_samples samples.  Options: headroom_db (0.1,
    mode "peak"), zero_crossings (32), kaiser_beta (9.0), rolloff (0.95) of the true-peak filter."""

    def __init__(self, rate=16000, target_lufs=-16.0, true_peak_db=-1.5, mode="loudness", max_rows=1024, max_samples=16000, **cfg):
        self.cfg = make_cfg(rate, target_lufs=target_lufs, true_peak_db=true_peak_db, mode=mode, **cfg)
        self.rate, self.max_rows, self.max_samples = int(rate), int(max_rows), int(max_samples)
        self.options = dict(target_lufs=float(target_lufs), true_peak_db=float(true_peak_db), mode=mode, **cfg)
        self.L = _lib.lib()
        h = ctypes.c_void_p()
        _lib.check(self.L.mkws_loudness_create(ctypes.byref(self.cfg), self.max_rows, self.max_samples, ctypes.byref(h)))
        self.h = h
        self.geometry = geometry(self.cfg)

    def close(self):
        if getattr(self, "h", None):
            self.L.mkws_loudness_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- what a call is given ------------------------------------------------------------------------------------------------------
    def _accept(self, audio):
        """What can be refused without a device call -> (is_np, the audio as a tensor, B, n)."""
        import torch
        is_np = not torch.is_tensor(audio)
        a = torch.from_numpy(np.ascontiguousarray(audio)) if is_np else audio
        if a.dtype not in (torch.float32, torch.int16):
            raise TypeError(f"audio must be float32 or int16, got {a.dtype}")
        if a.dim() not in (1, 2):
            raise ValueError("audio must be [n] or [B, n]")
        B, n = (1, a.shape[0]) if a.dim() == 1 else a.shape
        if B > self.max_rows or n > self.max_samples:
            raise ValueError(f"audio of {B} rows of {n} samples; the meter was created for {self.max_rows} rows of {self.max_samples}")
        return is_np, a, int(B), int(n)

    @staticmethod
    def _rows(a):
        """-> (host?, rank-1?, rows [B, n] on the device with unit sample stride and rows that do not overlap)."""
        host = not a.is_cuda
        d = a.cuda() if host else a
        rows = d[None] if d.dim() == 1 else d
        if rows.shape[1] > 1 and rows.stride(1) != 1 or (rows.shape[0] > 1 and rows.stride(0) < rows.shape[1]):
            rows = rows.contiguous()
        return host, a.dim() == 1, rows

    @staticmethod
    def _check_lengths(lengths, B, n):
        """None, a CUDA int64 tensor [B] (taken as it is: the kernels clamp it to [0, n]) or host integers [B] in [0, n]."""
        import torch
        if lengths is None:
            return None
        if torch.is_tensor(lengths) and lengths.is_cuda:
            if lengths.dtype != torch.int64 or tuple(lengths.shape) != (B,) or not lengths.is_contiguous():
                raise ValueError(f"lengths must be a contiguous int64 tensor [{B}]")
            return lengths
        host = np.asarray(lengths.numpy() if torch.is_tensor(lengths) else lengths)
        if host.shape != (B,) or host.dtype.kind not in "iu" or (B and (int(host.min()) < 0 or int(host.max()) > n)):
            raise ValueError(f"lengths must be {B} integers in [0, {n}]")
        return host.astype(np.int64)

    def _measure(self, rows, lengths):
        import torch
        B, n = rows.shape
        dev = rows.device
        if lengths is not None and not torch.is_tensor(lengths):
            lengths = torch.from_numpy(lengths).to(dev)
        elif lengths is not None and lengths.device != dev:
            raise ValueError("lengths must be on the device of audio")
        stats = torch.empty((B, 4), dtype=torch.float64, device=dev)
        counts = torch.empty((B, 4), dtype=torch.int32, device=dev)
        gain = torch.empty(B, dtype=torch.float32, device=dev)
        if B:
            with torch.cuda.device(dev):
                _lib.check(self.L.mkws_loudness_measure(
                    self.h, ctypes.c_void_p(rows.data_ptr()), int(rows.dtype == torch.int16), B, n, int(rows.stride(0)) if B > 1 else n,
                    ctypes.c_void_p(lengths.data_ptr()) if lengths is not None else None, ctypes.c_void_p(stats.data_ptr()),
                    ctypes.c_void_p(counts.data_ptr()), ctypes.c_void_p(gain.data_ptr()), _lib.current_stream_ptr()))
        return stats, counts, gain, lengths

    @staticmethod
    def _back(ts, is_np, host, one):
        out = []
        for t in ts:
            t = t[0] if one else t
            t = t.cpu() if host else t
            out.append(t.numpy() if is_np else t)
        return out

    # -- the four methods --------------------------------------------------------------------------------------------------------------
    def measure(self, audio, lengths=None):
        """audio: numpy array or tensor, [n] or [B, n], float32 or int16 PCM; lengths: the samples of every row that count (None = all).
        -> (stats float64 [B, 4] = loudness in LUFS, true peak, sample peak (both linear), mean square; counts int32 [B, 4] = blocks,
        blocks past the absolute gate, blocks past both gates, flags), [4] each for a rank-1 input.  A CUDA tensor stays on its device
        (rows may be strided; asynchronous on the current stream); anything else is uploaded and the results come back to the host."""
        is_np, a, B, n = self._accept(audio)
        lengths = self._check_lengths(lengths, B, n)
        host, one, rows = self._rows(a)
        stats, counts, _, _ = self._measure(rows, lengths)
        return tuple(self._back((stats, counts), is_np, host, one))

    def gains(self, audio, lengths=None):
        """The float32 gain of every row by the meter's mode ([B], or a scalar array for a rank-1 input); 1 for a row that could not be
        measured (flag FLAG_UNMEASURED of measure's counts)."""
        is_np, a, B, n = self._accept(audio)
        lengths = self._check_lengths(lengths, B, n)
        host, one, rows = self._rows(a)
        _, _, gain, _ = self._measure(rows, lengths)
        return self._back((gain,), is_np, host, one)[0]

    def normalize(self, audio, lengths=None, out=None):
        """float32 audio of the same kind and shape: row b times its gain (one rounding), 0 from lengths[b] on.  out: a CUDA float32
        tensor [B, n] with contiguous rows that overlap neither each other nor audio, on the device of audio.  (mkws_loudness_apply
        itself admits out == audio for float32 rows of equal strides; this wrapper refuses every overlap, the exact one included.  With
        host audio and an out, the result is written to out AND comes back as a host array of audio's kind.)"""
        import torch
        is_np, a, B, n = self._accept(audio)
        lengths = self._check_lengths(lengths, B, n)
        if out is not None:
            if not torch.is_tensor(out) or not out.is_cuda or (a.is_cuda and out.device != a.device) or out.dtype != torch.float32 \
                    or tuple(out.shape) != (B, n) or (n > 1 and out.stride(1) != 1) or (B > 1 and out.stride(0) < n):
                raise ValueError(f"out must be a CUDA float32 tensor [{B}, {n}] with contiguous rows that do not overlap, on the device of audio")
            if a.is_cuda and a.device == out.device and B and n:
                rows2 = a[None] if a.dim() == 1 else a
                reach = sum((size - 1) * abs(stride) for size, stride in zip(rows2.shape, rows2.stride())) + 1
                lo, hi = out.data_ptr(), out.data_ptr() + 4 * ((B - 1) * out.stride(0) + n)
                alo, ahi = rows2.data_ptr(), rows2.data_ptr() + rows2.element_size() * reach
                if min(rows2.stride()) < 0 or (lo < ahi and alo < hi):
                    raise ValueError("out must not overlap audio")
        host, one, rows = self._rows(a)
        if out is not None and out.device != rows.device:
            raise ValueError("out must be on the device the audio was uploaded to")
        _, _, gain, lengths = self._measure(rows, lengths)
        if out is None:
            out = torch.empty((B, n), dtype=torch.float32, device=rows.device)
        if B and n:
            with torch.cuda.device(rows.device):
                _lib.check(self.L.mkws_loudness_apply(
                    self.h, ctypes.c_void_p(rows.data_ptr()), int(rows.dtype == torch.int16), B, n, int(rows.stride(0)) if B > 1 else n,
                    ctypes.c_void_p(lengths.data_ptr()) if lengths is not None else None, ctypes.c_void_p(gain.data_ptr()),
                    ctypes.c_void_p(out.data_ptr()), int(out.stride(0)) if B > 1 else n, _lib.current_stream_ptr()))
        return self._back((out,), is_np, host, one)[0]
