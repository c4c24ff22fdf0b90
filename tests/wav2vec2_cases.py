"""Shared cases of tests/test_wav2vec2_cpu.py and tests/test_wav2vec2_gpu.py: the three small configurations, the golden files, seeded
audio, and the float64 / float32 evaluations of wav2vec2.reference_forward on the CPU, each computed once and shared read-only.

The configurations are the smallest at which each route can go wrong: `tiny` (everything a multiple of 4: the vector GEMM route, an
even positional kernel), `mid` (unequal conv_dim, an odd positional kernel, head_dim 16, an FFN width that is no multiple of 64),
`ragged` (nothing a multiple of 4: the GEMM's guarded route, head_dim 10, one channel pair per positional group of 6)."""
import functools
import os

import numpy as np
import torch

from multilingual_kws_amd import wav2vec2

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CONFIGS = {
    "tiny": wav2vec2.Config(conv_dim=(16,) * 7, hidden_size=32, num_attention_heads=4, intermediate_size=64, num_hidden_layers=2,
                            num_conv_pos_embeddings=16, num_conv_pos_embedding_groups=4),
    "mid": wav2vec2.Config(conv_dim=(24, 40, 40, 40, 40, 40, 56), hidden_size=96, num_attention_heads=6, intermediate_size=200,
                           num_hidden_layers=3, num_conv_pos_embeddings=15, num_conv_pos_embedding_groups=3),
    "ragged": wav2vec2.Config(conv_dim=(6, 10, 10, 10, 10, 10, 14), hidden_size=30, num_attention_heads=3, intermediate_size=50,
                              num_hidden_layers=2, num_conv_pos_embeddings=5, num_conv_pos_embedding_groups=5),
}
PARAM_COUNTS = {"tiny": 26160, "mid": 306199, "ragged": 16945}
GOLDEN_FILES = {"tiny": "wav2vec2_golden.npz", "ragged": "wav2vec2_golden.npz", "mid": "wav2vec2_golden_mid.npz"}
GOLDEN_LENGTHS = (400, 1000, 16000)
LENGTHS = (400, 721, 1000, 4000, 16000)          # T = 1, 2, 2, 12, 49
FRAMES = {399: 0, 400: 1, 721: 2, 1000: 2, 4000: 12, 16000: 49, 16001: 49}
BATCHES = (1, 3)                                  # (the handle takes a whole batch in one pass: there is no clip-per-pass boundary)
MAX_BATCH = 3
FACTOR = 4.0                                      # the device may be this many times the float32 reference's own error away from float64


@functools.lru_cache(maxsize=None)
def golden(name):
    """{key without the configuration's prefix: array}, parameters and audio widened to float32 (they are stored as float16, exactly)."""
    with np.load(os.path.join(GOLDEN, GOLDEN_FILES[name])) as z:
        out = {k[len(name) + 1:]: z[k] for k in z.files if k.startswith(name + "_")}
    for k in out:
        if out[k].dtype == np.float16:
            out[k] = out[k].astype(np.float32)
        out[k].setflags(write=False)
    return out


def params(name):
    return golden(name)["params"]


@functools.lru_cache(maxsize=None)
def audio(n, B, seed=0):
    """[B, n] float32: per clip a tone of its own frequency and level over noise, with an offset, so that the processor's mean and
    variance matter and no two clips agree."""
    rng = np.random.default_rng(1000 * seed + 10 * n + B)
    t = np.arange(n) / 16000.0
    a = rng.uniform(0.1, 0.6, (B, 1)) * np.sin(2 * np.pi * rng.uniform(100, 3000, (B, 1)) * t) + 0.1 * rng.standard_normal((B, n)) + rng.uniform(-0.1, 0.1, (B, 1))
    a = a.astype(np.float32)
    a.setflags(write=False)
    return a


def rel_err(got, want):
    """max |got - want| / max |want| in float64."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    return float(np.abs(got - want).max() / np.abs(want).max())


class Case:
    """One evaluation: the float64 reference (hidden, embedding, taps) and E32, the float32 reference's distance from it, relative to
    max |float64|: for the last hidden state (e32), the embedding (e32_embed) and every tap stage (e32_taps)."""

    def __init__(self, config, blob, clips, normalize=True):
        r64 = wav2vec2.reference_forward(config, blob, np.array(clips), normalize=normalize, taps=True, dtype=torch.float64)
        r32 = wav2vec2.reference_forward(config, blob, np.array(clips), normalize=normalize, taps=True, dtype=torch.float32)
        self.audio = clips
        self.hidden = r64.last_hidden_state.numpy()
        self.embed = r64.embedding.numpy()
        self.taps = [t.contiguous().numpy() for t in r64.taps]
        self.e32 = rel_err(r32.last_hidden_state.numpy(), self.hidden)
        self.e32_embed = rel_err(r32.embedding.numpy(), self.embed)
        self.e32_taps = [rel_err(a.numpy(), b) for a, b in zip(r32.taps, self.taps)]


@functools.lru_cache(maxsize=None)
def case(name, n, B, normalize=True):
    return Case(CONFIGS[name], params(name), audio(n, B), normalize)


@functools.lru_cache(maxsize=None)
def golden_case(name, n):
    return Case(CONFIGS[name], params(name), golden(name)[f"{n}_audio"])
