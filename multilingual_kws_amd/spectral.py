"""Device mfcc / average feature extractor: thin host wrapper over mkws_spectral_* (include/mkws.h), the reference's non-micro pipeline
(tf_v1_speechcommands/input_data_fix_bg.py:444-475)."""
import ctypes

import numpy as np

from . import _lib

MFCC, AVERAGE = 0, 1
_MODES = {"mfcc": MFCC, "average": AVERAGE}
_TABLE_IDS = dict(window=(0, np.float32), mel_weights=(1, np.float32), band_mapper=(2, np.int32), dct=(3, np.float32), scalars=(4, np.int32))
_SCALARS = ("window", "stride", "fft_size", "bins", "width", "channels", "start_index", "end_index")


def make_cfg(**over):
    """mkws_spectral_default_cfg with overrides; mode takes "mfcc" / "average" or the integer."""
    cfg = _lib.SpectralCfg()
    _lib.lib().mkws_spectral_default_cfg(ctypes.byref(cfg))
    for k, v in over.items():
        if not hasattr(cfg, k):
            raise TypeError(f"unknown spectral option {k!r}")
        if k == "mode" and isinstance(v, str):
            if v not in _MODES:
                raise ValueError(f'mode {v!r} (should be "mfcc" or "average")')
            v = _MODES[v]
        setattr(cfg, k, int(v) if isinstance(getattr(cfg, k), int) else float(v))
    return cfg


def geometry(cfg):
    """Host only -> (fft_size, bins, width); MkwsError for a configuration the library refuses, naming the field."""
    f, b, w = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    _lib.check(_lib.lib().mkws_spectral_geometry(ctypes.byref(cfg), ctypes.byref(f), ctypes.byref(b), ctypes.byref(w)))
    return f.value, b.value, w.value


def num_frames(cfg, n_samples):
    return _lib.check(_lib.lib().mkws_spectral_num_frames(ctypes.byref(cfg), int(n_samples)))


def host_table(cfg, name):
    """Host only (works without a GPU): one of the tables the library builds for cfg."""
    which, dt = _TABLE_IDS[name]
    L = _lib.lib()
    n = _lib.check(L.mkws_spectral_host_table(ctypes.byref(cfg), which, None, 0))
    buf = np.zeros(n // np.dtype(dt).itemsize, dtype=dt)
    _lib.check(L.mkws_spectral_host_table(ctypes.byref(cfg), which, buf.ctypes.data, n))
    return buf


def host_scalars(cfg):
    return dict(zip(_SCALARS, host_table(cfg, "scalars").tolist()))


def windows(n_samples, window_samples, hop_samples):
    """The num_windows of SpectralFrontend.stream."""
    return 0 if n_samples < window_samples else 1 + (n_samples - window_samples) // hop_samples


class SpectralFrontend:
    """One configured device feature extractor (tables uploaded once).  All tensors are torch CUDA tensors."""

    def __init__(self, max_samples=16000, **cfg_over):
        self.cfg = make_cfg(**cfg_over)
        self.L = _lib.lib()
        self.fft_size, self.bins, self.width = geometry(self.cfg)
        self.channels = self.cfg.filterbank_channels if self.cfg.mode == MFCC else 0
        h = ctypes.c_void_p()
        _lib.check(self.L.mkws_spectral_create(ctypes.byref(self.cfg), int(max_samples), ctypes.byref(h)))
        self.h = h
        self.max_samples = int(max_samples)

    def close(self):
        if getattr(self, "h", None):
            self.L.mkws_spectral_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def forward(self, audio, want_power=False, want_mel=False, out=None):
        """audio: CUDA tensor [B, n] or [n], float32 in [-1, 1] or int16 PCM -> float32 [B, frames, width]; with want_power also the
        squared-magnitude spectrogram [B, frames, bins], with want_mel (mfcc mode) the filterbank outputs before the log
        [B, frames, channels]: (feat, power, mel), the taps not asked for left out."""
        import torch
        if not torch.is_tensor(audio) or not audio.is_cuda:
            raise ValueError("SpectralFrontend.forward needs a CUDA tensor (no CPU path)")
        if want_mel and self.cfg.mode != MFCC:
            raise ValueError("SpectralFrontend.forward: want_mel needs the mfcc mode")
        B, n, F = check_forward(self.cfg, audio.device, audio, out, self.max_samples)
        if audio.dim() == 1:
            audio = audio[None]
        audio = audio.contiguous()
        dev = audio.device
        feat = out if out is not None else torch.empty((B, F, self.width), dtype=torch.float32, device=dev)
        power = torch.empty((B, F, self.bins), dtype=torch.float32, device=dev) if want_power else None
        mel = torch.empty((B, F, self.channels), dtype=torch.float32, device=dev) if want_mel else None
        if B > 0 and F > 0:
            fn = self.L.mkws_spectral_forward_f32 if audio.dtype == torch.float32 else self.L.mkws_spectral_forward_i16
            with torch.cuda.device(dev):
                _lib.check(fn(self.h, ctypes.c_void_p(audio.data_ptr()), B, n, ctypes.c_void_p(feat.data_ptr()),
                              ctypes.c_void_p(power.data_ptr()) if want_power else None, ctypes.c_void_p(mel.data_ptr()) if want_mel else None,
                              _lib.current_stream_ptr()))
        got = (feat,) + ((power,) if want_power else ()) + ((mel,) if want_mel else ())
        return got if len(got) > 1 else feat

    def stream(self, audio, window_samples, hop_samples):
        """One long recording [n] float32 -> [num_windows, frames, width], window w covering samples [w * hop, w * hop + window): every
        frame computed once, row w bit-equal to forward() on the cut window."""
        import torch
        if not torch.is_tensor(audio) or not audio.is_cuda:
            raise ValueError("SpectralFrontend.stream: audio must be a CUDA tensor (no CPU path)")
        n, F, nw = check_stream(self.cfg, audio.device, audio, window_samples, hop_samples, self.max_samples)
        audio = audio.contiguous()
        feat = torch.empty((nw, F, self.width), dtype=torch.float32, device=audio.device)
        if nw > 0 and F > 0:
            with torch.cuda.device(audio.device):
                got = _lib.check(self.L.mkws_spectral_stream_f32(self.h, ctypes.c_void_p(audio.data_ptr()), n, int(window_samples), int(hop_samples),
                                                                 ctypes.c_void_p(feat.data_ptr()), nw, _lib.current_stream_ptr()))
            assert got == nw
        return feat


def _describe(t):
    import torch
    return f"{t.dtype} {tuple(t.shape)} (strides {t.stride()}) on {t.device}" if torch.is_tensor(t) else type(t).__name__


def check_forward(cfg, device, audio, out=None, max_samples=None):
    """What SpectralFrontend.forward refuses, decided before any device call: audio a float32 or int16 tensor [B, n] or [n] on `device` (a
    strided view is made contiguous by the wrapper; TypeError for another dtype) of at most max_samples samples a row; `out` (if given) a
    contiguous float32 tensor [rows >= B, frames, width] on `device`.  -> (B, n, frames).  ValueError otherwise."""
    import torch
    if not torch.is_tensor(audio) or audio.dim() not in (1, 2) or audio.device != device:
        raise ValueError(f"SpectralFrontend.forward: audio must be a tensor [B, n] or [n] on {device}, got {_describe(audio)}")
    if audio.dtype not in (torch.float32, torch.int16):
        raise TypeError(f"audio must be float32 or int16, got {audio.dtype}")
    B, n = (1, int(audio.shape[0])) if audio.dim() == 1 else (int(audio.shape[0]), int(audio.shape[1]))
    if max_samples is not None and n > int(max_samples):
        raise ValueError(f"SpectralFrontend.forward: audio rows of {n} samples exceed the handle's max_samples {int(max_samples)}")
    F = num_frames(cfg, n)
    W = cfg.num_features
    if out is not None and (not torch.is_tensor(out) or out.dim() != 3 or tuple(out.shape[1:]) != (F, W) or out.shape[0] < B or out.dtype != torch.float32
                            or not out.is_contiguous() or out.device != device):
        raise ValueError(f"SpectralFrontend.forward: out must be a contiguous float32 tensor [{B}, {F}, {W}] on {device}, got {_describe(out)}")
    return B, n, F


def check_stream(cfg, device, audio, window_samples, hop_samples, max_samples=None):
    """What SpectralFrontend.stream refuses, decided before any device call: audio a float32 vector [n] on `device` (a strided view is made
    contiguous by the wrapper) of at most max_samples samples, a window of at least one sample and a hop that is a positive multiple of
    the frame stride.  -> (n, frames, num_windows).  ValueError otherwise."""
    import torch
    if not torch.is_tensor(audio) or audio.dim() != 1 or audio.dtype != torch.float32 or audio.device != device:
        raise ValueError(f"SpectralFrontend.stream: audio must be a float32 vector [n] on {device}, got {_describe(audio)}")
    if int(window_samples) < 1:
        raise ValueError(f"SpectralFrontend.stream: window_samples={window_samples} must be positive")
    if int(hop_samples) < 1 or int(hop_samples) % cfg.window_stride_samples != 0:
        raise ValueError(f"SpectralFrontend.stream: hop_samples={hop_samples} must be a positive multiple of the frame stride {cfg.window_stride_samples}")
    n = int(audio.shape[0])
    if max_samples is not None and n > int(max_samples):
        raise ValueError(f"SpectralFrontend.stream: audio of {n} samples exceeds the handle's max_samples {int(max_samples)}")
    return n, num_frames(cfg, int(window_samples)), windows(n, int(window_samples), int(hop_samples))
