"""The wav2vec 2.0 encoder the reference uses as a clip embedding (notebooks/dataperf_wav2vec2.py:43-58: Wav2Vec2Processor +
Wav2Vec2Model, last hidden state max-pooled over time): configuration, parameter blob, loaders, the specification in plain torch
operators (reference_forward) and the device wrapper over mkws_w2v2_* (include/mkws.h).

Parameters are a flat float32 blob with the names, layouts and order of Hugging Face's Wav2Vec2Model state dict, masked_spec_embed
left out (manifest()).  Nothing here fetches anything; transformers is not imported."""
import contextlib
import ctypes
import dataclasses
import json
import os
from collections import namedtuple

import numpy as np

from . import _lib

CONV_KERNEL = (10, 3, 3, 3, 3, 2, 2)
CONV_STRIDE = (5, 2, 2, 2, 2, 2, 2)
PROCESSOR_EPS = 1e-7
GROUP_NORM_EPS = 1e-5
MIN_SAMPLES = 400

Forward = namedtuple("Forward", "last_hidden_state embedding extract_features taps")


@dataclasses.dataclass(frozen=True)
class Config:
    """The fields of Hugging Face's Wav2Vec2Config the encoder depends on; the defaults are facebook/wav2vec2-base(-960h)."""
    conv_dim: tuple = (512,) * 7
    conv_kernel: tuple = CONV_KERNEL
    conv_stride: tuple = CONV_STRIDE
    hidden_size: int = 768
    num_hidden_layers: int = 12
    num_attention_heads: int = 12
    intermediate_size: int = 3072
    num_conv_pos_embeddings: int = 128
    num_conv_pos_embedding_groups: int = 16
    layer_norm_eps: float = 1e-5
    feat_extract_norm: str = "group"
    conv_bias: bool = False
    do_stable_layer_norm: bool = False
    hidden_act: str = "gelu"
    feat_extract_activation: str = "gelu"

    @classmethod
    def base(cls):
        return cls()

    @classmethod
    def from_hf_dict(cls, d):
        """A config.json dict -> Config; keys it lacks take Wav2Vec2Config's defaults, keys the encoder does not depend on are ignored."""
        known = {f.name for f in dataclasses.fields(cls)}
        kw = {k: v for k, v in dict(d).items() if k in known}
        for k in ("conv_dim", "conv_kernel", "conv_stride"):
            if k in kw:
                kw[k] = tuple(int(v) for v in kw[k])
        return cls(**kw)

    def to_c(self):
        """-> _lib.W2v2Cfg.  ValueError for fields that do not even fit the struct; everything else is the library's to refuse."""
        if len(self.conv_dim) != 7 or len(self.conv_kernel) != 7 or len(self.conv_stride) != 7:
            raise ValueError(f"a wav2vec 2.0 feature encoder of 7 layers, got conv_dim {self.conv_dim}, conv_kernel {self.conv_kernel}, conv_stride {self.conv_stride}")
        c = _lib.W2v2Cfg()
        for i in range(7):
            c.conv_dim[i], c.conv_kernel[i], c.conv_stride[i] = int(self.conv_dim[i]), int(self.conv_kernel[i]), int(self.conv_stride[i])
        c.hidden_size, c.num_hidden_layers, c.num_attention_heads = int(self.hidden_size), int(self.num_hidden_layers), int(self.num_attention_heads)
        c.intermediate_size = int(self.intermediate_size)
        c.num_conv_pos_embeddings, c.num_conv_pos_embedding_groups = int(self.num_conv_pos_embeddings), int(self.num_conv_pos_embedding_groups)
        c.layer_norm_eps = float(self.layer_norm_eps)
        c.group_norm = int(self.feat_extract_norm == "group")
        c.conv_bias, c.stable_layer_norm = int(bool(self.conv_bias)), int(bool(self.do_stable_layer_norm))
        c.exact_gelu = int(self.hidden_act == "gelu" and self.feat_extract_activation == "gelu")
        return c


def _refused():
    return ValueError(_lib.lib().mkws_last_error().decode("utf-8", "replace"))


def param_count(config):
    """Floats of the blob.  ValueError for a configuration the build refuses (host-only call, no GPU needed)."""
    n = int(_lib.lib().mkws_w2v2_param_count(ctypes.byref(config.to_c())))
    if n == 0:
        raise _refused()
    return n


def manifest(config):
    """[{name, shape, offset, count}] straight from the C library: Hugging Face's state-dict names, layouts and order."""
    L, c = _lib.lib(), config.to_c()
    n = L.mkws_w2v2_weight_manifest(ctypes.byref(c), None, 0)
    if n < 0:
        raise _refused()
    buf = ctypes.create_string_buffer(n + 1)
    _lib.check(L.mkws_w2v2_weight_manifest(ctypes.byref(c), buf, n + 1))
    return json.loads(buf.value.decode("utf-8"))["tensors"]


def num_frames(config, n_samples):
    """Frames of a clip of n_samples; 0 below 400 samples."""
    return max(0, int(_lib.lib().mkws_w2v2_num_frames(ctypes.byref(config.to_c()), int(n_samples))))


def unpack(config, params):
    """blob -> {state-dict name: float32 view of its shape}."""
    params = np.asarray(params, dtype=np.float32)
    if params.ndim != 1 or params.shape[0] != param_count(config):
        raise ValueError(f"parameter blob of shape {params.shape}, this configuration needs {param_count(config)} floats")
    return {t["name"]: params[t["offset"]:t["offset"] + t["count"]].reshape(t["shape"]) for t in manifest(config)}


def synthetic_weights(config, seed=1234):
    """Seeded parameters, identical on every machine (NumPy's PCG64, one draw per tensor in manifest order), chosen to tell: LayerNorm
    and GroupNorm gammas U(0.5, 1.5), every bias and beta N(0, 0.1), kernels N(0, gain / fan_in) with the gain that keeps a GELU
    layer's output at unit scale, the positional kernel's direction v N(0, 1) and its magnitudes g = sqrt(H / K) * U(0.8, 1.2), so
    that activations stay O(1) through all layers at the base configuration."""
    rng = np.random.default_rng(seed)
    blob = np.zeros(param_count(config), dtype=np.float32)
    H, K = config.hidden_size, config.num_conv_pos_embeddings
    for t in manifest(config):
        name, shape = t["name"], tuple(t["shape"])
        v = blob[t["offset"]:t["offset"] + t["count"]].reshape(shape)
        if name.endswith("original0"):
            v[...] = np.float32(np.sqrt(H / K)) * rng.uniform(0.8, 1.2, shape).astype(np.float32)
        elif name.endswith("original1"):
            v[...] = rng.standard_normal(shape, dtype=np.float32)
        elif name.endswith("layer_norm.weight"):
            v[...] = rng.uniform(0.5, 1.5, shape).astype(np.float32)
        elif name.endswith(".bias"):
            v[...] = np.float32(0.1) * rng.standard_normal(shape, dtype=np.float32)
        else:
            fan_in = int(np.prod(shape[1:]))
            gain = 2.0 if ".conv.weight" in name or "intermediate_dense" in name else 1.0
            v[...] = np.float32(np.sqrt(gain / fan_in)) * rng.standard_normal(shape, dtype=np.float32)
    return blob


# ---------------------------------------------------------------------------------------------- loaders
_OLD_NORM = {"encoder.pos_conv_embed.conv.weight_g": "encoder.pos_conv_embed.conv.parametrizations.weight.original0",
             "encoder.pos_conv_embed.conv.weight_v": "encoder.pos_conv_embed.conv.parametrizations.weight.original1"}


def from_state_dict(config, mapping):
    """{name: array or tensor} under Hugging Face's names -> blob.  A `wav2vec2.` prefix (a checkpoint of Wav2Vec2ForCTC or
    ForPreTraining) is dropped, both spellings of the weight-norm tensors are taken (parametrizations.weight.original0/1 and the older
    weight_g / weight_v), tensors the encoder does not own (masked_spec_embed, heads, the quantiser) are left aside.  ValueError for a
    missing tensor or a wrong shape."""
    named = {}
    for k, v in mapping.items():
        k = k[len("wav2vec2."):] if k.startswith("wav2vec2.") else k
        named[_OLD_NORM.get(k, k)] = v
    blob = np.zeros(param_count(config), dtype=np.float32)
    for t in manifest(config):
        if t["name"] not in named:
            raise ValueError(f"the state dict has no '{t['name']}'")
        v = named[t["name"]]
        v = v.detach().cpu().numpy() if hasattr(v, "detach") else np.asarray(v)
        if list(v.shape) != list(t["shape"]):
            raise ValueError(f"{t['name']}: shape {list(v.shape)}, this configuration needs {t['shape']}")
        blob[t["offset"]:t["offset"] + t["count"]] = v.astype(np.float32).reshape(-1)
    return blob


def from_pretrained_dir(path):
    """A directory as save_pretrained writes it -> (Config, blob): config.json plus pytorch_model.bin (torch.load) or model.safetensors
    (only where the safetensors package is importable).  Reads local files only."""
    with open(os.path.join(path, "config.json")) as f:
        config = Config.from_hf_dict(json.load(f))
    bin_path, st_path = os.path.join(path, "pytorch_model.bin"), os.path.join(path, "model.safetensors")
    if os.path.exists(bin_path):
        import torch
        state = torch.load(bin_path, map_location="cpu", weights_only=True)
    elif os.path.exists(st_path):
        try:
            from safetensors.numpy import load_file
        except ImportError as e:
            raise ImportError(f"{st_path} needs the safetensors package; convert it to pytorch_model.bin where that is installed") from e
        state = load_file(st_path)
    else:
        raise FileNotFoundError(f"{path} holds neither pytorch_model.bin nor model.safetensors")
    return config, from_state_dict(config, state)


# ---------------------------------------------------------------------------------------------- the specification
def reference_weights(config, params, device, dtype):
    """The blob as {state-dict name: tensor on `device` in `dtype`}: what reference_forward prepares on every call unless it is given."""
    import torch
    return {k: torch.from_numpy(np.array(v)).to(device, dtype) for k, v in unpack(config, params).items()}      # (a copy: the blob may be read-only)


def reference_forward(config, params, audio, normalize=True, taps=False, dtype=None, weights=None):
    """The specification of the device forward in plain torch operators, on the device of `audio` (CPU for a numpy array), in `dtype`
    (float64 unless given).  audio [B, n] -> Forward(last_hidden_state [B,T,H], embedding [B,H] = max over the T frames,
    extract_features [B,T,conv_dim[6]] = the projection's LayerNorm output, taps = the stages of mkws_w2v2_tap in order, or None).
    weights: reference_weights(config, params, audio.device, dtype) prepared by the caller (params is then not read)."""
    import torch
    import torch.nn.functional as F
    dtype = dtype or torch.float64
    if tuple(config.conv_kernel) != CONV_KERNEL or tuple(config.conv_stride) != CONV_STRIDE or config.to_c().exact_gelu != 1 or \
            config.feat_extract_norm != "group" or config.conv_bias or config.do_stable_layer_norm:
        raise ValueError("reference_forward: a configuration outside the specification (kernels, strides, group norm, no conv bias, post-LN, exact GELU)")
    audio = audio if torch.is_tensor(audio) else torch.from_numpy(np.array(audio))
    if audio.dim() != 2 or audio.shape[1] < MIN_SAMPLES:
        raise ValueError(f"audio must be [B, n >= {MIN_SAMPLES}], got {tuple(audio.shape)}")
    dev = audio.device
    w = weights if weights is not None else reference_weights(config, params, dev, dtype)
    eps, H = float(config.layer_norm_eps), config.hidden_size
    stages = []
    x = audio.to(dtype)
    if normalize:
        mean = x.mean(dim=1, keepdim=True)
        var = ((x - mean) ** 2).mean(dim=1, keepdim=True)
        x = (x - mean) / torch.sqrt(var + PROCESSOR_EPS)
    stages.append(x)
    h = x[:, None, :]
    for i in range(7):
        p = f"feature_extractor.conv_layers.{i}"
        h = F.conv1d(h, w[p + ".conv.weight"], stride=CONV_STRIDE[i])
        if i == 0:
            h = F.group_norm(h, h.shape[1], w[p + ".layer_norm.weight"], w[p + ".layer_norm.bias"], GROUP_NORM_EPS)
        h = F.gelu(h)
        stages.append(h.transpose(1, 2))
    h = h.transpose(1, 2)
    C6 = h.shape[-1]
    feat = F.layer_norm(h, (C6,), w["feature_projection.layer_norm.weight"], w["feature_projection.layer_norm.bias"], eps)
    h = F.linear(feat, w["feature_projection.projection.weight"], w["feature_projection.projection.bias"])
    stages.append(h)
    K, G = config.num_conv_pos_embeddings, config.num_conv_pos_embedding_groups
    g, v = w["encoder.pos_conv_embed.conv.parametrizations.weight.original0"], w["encoder.pos_conv_embed.conv.parametrizations.weight.original1"]
    wn = g * v / torch.sqrt((v * v).sum(dim=(0, 1), keepdim=True))
    y = F.conv1d(h.transpose(1, 2), wn, w["encoder.pos_conv_embed.conv.bias"], padding=K // 2, groups=G)
    if K % 2 == 0:
        y = y[:, :, :-1]
    h = h + F.gelu(y).transpose(1, 2)
    h = F.layer_norm(h, (H,), w["encoder.layer_norm.weight"], w["encoder.layer_norm.bias"], eps)
    stages.append(h)
    heads = config.num_attention_heads
    d = H // heads
    B, T = h.shape[0], h.shape[1]
    for l in range(config.num_hidden_layers):
        p = f"encoder.layers.{l}"
        split = lambda z: z.view(B, T, heads, d).transpose(1, 2)
        q = split(F.linear(h, w[p + ".attention.q_proj.weight"], w[p + ".attention.q_proj.bias"]) * d ** -0.5)
        k = split(F.linear(h, w[p + ".attention.k_proj.weight"], w[p + ".attention.k_proj.bias"]))
        vv = split(F.linear(h, w[p + ".attention.v_proj.weight"], w[p + ".attention.v_proj.bias"]))
        a = torch.softmax(q @ k.transpose(-1, -2), dim=-1) @ vv
        a = F.linear(a.transpose(1, 2).reshape(B, T, H), w[p + ".attention.out_proj.weight"], w[p + ".attention.out_proj.bias"])
        h = F.layer_norm(h + a, (H,), w[p + ".layer_norm.weight"], w[p + ".layer_norm.bias"], eps)
        f = F.gelu(F.linear(h, w[p + ".feed_forward.intermediate_dense.weight"], w[p + ".feed_forward.intermediate_dense.bias"]))
        f = F.linear(f, w[p + ".feed_forward.output_dense.weight"], w[p + ".feed_forward.output_dense.bias"])
        h = F.layer_norm(h + f, (H,), w[p + ".final_layer_norm.weight"], w[p + ".final_layer_norm.bias"], eps)
        stages.append(h)
    return Forward(h, h.amax(dim=1), feat, stages if taps else None)


# ---------------------------------------------------------------------------------------------- the device wrapper
def check_audio(audio, device, max_batch, max_samples, who="Wav2Vec2.forward"):
    """What the wrapper refuses, decided before any device call: audio must be a contiguous float32 tensor [B, n] on `device` with
    B <= max_batch and 400 <= n <= max_samples.  -> (B, n).  ValueError otherwise."""
    import torch
    if not torch.is_tensor(audio) or audio.dim() != 2 or audio.dtype != torch.float32 or audio.device != device:
        got = f"{audio.dtype} {tuple(audio.shape)} on {audio.device}" if torch.is_tensor(audio) else type(audio).__name__
        raise ValueError(f"{who}: audio must be a float32 tensor [B, samples] on {device}, got {got}")
    if not audio.is_contiguous():
        raise ValueError(f"{who}: audio must be contiguous, got strides {tuple(audio.stride())} for shape {tuple(audio.shape)}")
    B, n = int(audio.shape[0]), int(audio.shape[1])
    if B > int(max_batch):
        raise _lib.MkwsValueError(f"{who}: batch {B} above max_batch = {int(max_batch)}")
    if not MIN_SAMPLES <= n <= int(max_samples):
        raise _lib.MkwsValueError(f"{who}: {n} samples outside [{MIN_SAMPLES}, max_samples = {int(max_samples)}]")
    return B, n


class Wav2Vec2:
    """The encoder on the device.  `params`: the blob (manifest order).  All clips of a call have the same length; `normalize` is the
    processor's do_normalize (an attribute: it may be switched between calls)."""

    def __init__(self, config, params, max_batch=32, max_samples=16000, device=None, normalize=True):
        import torch
        self.L = _lib.lib()
        self.config = config
        params = np.ascontiguousarray(params, dtype=np.float32)
        if params.ndim != 1:
            raise ValueError(f"params must be one flat blob, got shape {params.shape}")
        self.device = _lib.indexed_device(device) if torch.cuda.is_available() else torch.device(device if device is not None else "cuda:0")
        h = ctypes.c_void_p()
        # (without a device the library still checks the configuration and the blob first, then says MKWS_ERR_NO_DEVICE)
        with torch.cuda.device(self.device) if torch.cuda.is_available() else contextlib.nullcontext():
            _lib.check(self.L.mkws_w2v2_create(ctypes.byref(config.to_c()), params.ctypes.data, params.shape[0], int(max_batch), int(max_samples), ctypes.byref(h)))
        self.h = h
        self.max_batch, self.max_samples = int(max_batch), int(max_samples)
        self.hidden_size = int(config.hidden_size)
        self.normalize = bool(normalize)          # the processor's do_normalize; False takes the audio as given

    @classmethod
    def from_pretrained_dir(cls, path, max_batch=32, max_samples=16000, device=None):
        config, params = from_pretrained_dir(path)
        return cls(config, params, max_batch=max_batch, max_samples=max_samples, device=device)

    def close(self):
        if getattr(self, "h", None):
            self.L.mkws_w2v2_destroy(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _checked(self, audio, who):
        if getattr(self, "h", None) is None:
            raise ValueError(f"{who}: the model is closed")
        return check_audio(audio, self.device, self.max_batch, self.max_samples, who)

    def _forward(self, audio, who, want_hidden, want_embed):
        import torch
        B, n = self._checked(audio, who)
        T, H = num_frames(self.config, n), self.hidden_size
        with torch.cuda.device(self.device):
            hidden = torch.empty((B, T, H), dtype=torch.float32, device=self.device) if want_hidden else None
            embed = torch.empty((B, H), dtype=torch.float32, device=self.device) if want_embed else None
            ptr = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None and t.numel() else None
            if B:
                _lib.check(self.L.mkws_w2v2_forward(self.h, ctypes.c_void_p(audio.data_ptr()), B, n, int(bool(self.normalize)), ptr(hidden), ptr(embed),
                                                    _lib.current_stream_ptr()))
        return hidden, embed

    def forward(self, audio):
        """audio: contiguous float32 CUDA [B, n] -> the last hidden state, CUDA [B, T, H]."""
        return self._forward(audio, "Wav2Vec2.forward", True, False)[0]

    def embed(self, audio):
        """-> the clip embedding of the reference: the maximum of the last hidden state over the T frames, CUDA [B, H]."""
        return self._forward(audio, "Wav2Vec2.embed", False, True)[1]

    def forward_embed(self, audio):
        """-> (last hidden state [B, T, H], embedding [B, H]) of one pass."""
        return self._forward(audio, "Wav2Vec2.forward_embed", True, True)

    def tap_shape(self, B, n, stage):
        stage, c = int(stage), self.config
        if not 0 <= stage <= 9 + c.num_hidden_layers:
            raise ValueError(f"Wav2Vec2.tap: stage {stage} outside [0, {9 + c.num_hidden_layers}]")
        if stage == 0:
            return (B, n)
        if stage <= 7:
            t = n
            for i in range(stage):
                t = (t - CONV_KERNEL[i]) // CONV_STRIDE[i] + 1
            return (B, t, int(c.conv_dim[stage - 1]))
        return (B, num_frames(c, n), self.hidden_size)

    def tap(self, audio, stage):
        """The chain stopped after `stage` (mkws_w2v2_tap): 0 the normalised audio; 1..7 the convolution layers [B, T_i, C_i]; 8 the
        projection; 9 positional convolution + LayerNorm; 10 + l transformer layer l."""
        import torch
        B, n = self._checked(audio, "Wav2Vec2.tap")
        shape = self.tap_shape(B, n, stage)
        with torch.cuda.device(self.device):
            out = torch.empty(shape, dtype=torch.float32, device=self.device)
            if B:
                _lib.check(self.L.mkws_w2v2_tap(self.h, ctypes.c_void_p(audio.data_ptr()), B, n, int(bool(self.normalize)), int(stage),
                                                ctypes.c_void_p(out.data_ptr()), _lib.current_stream_ptr()))
        return out
