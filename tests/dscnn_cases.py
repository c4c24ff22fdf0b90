"""Inputs and float64 references shared by tests/test_dscnn_cpu.py and tests/test_dscnn_gpu.py.

Uniform-noise spectrograms are useless for the DS-CNN: after the average pool every clip's features nearly coincide and all clips fall
in one class, so a kernel that read the wrong clip would still pass.  The clips here are dscnn.structured_clips (Gaussian blobs in time x
frequency over 0..60 noise, floored), drawn from seeds other than the one the synthetic BatchNorm statistics were calibrated on;
test_dscnn_cpu.py asserts on the reference alone that they keep every ReLU data-dependent, spread over the classes and keep any two
clips' logits apart."""
import functools

import numpy as np

from multilingual_kws_amd import dscnn

LABEL_COUNTS = (2, 7, 12, 64)
BATCHES = (1, 2, 3, 5, 67)
PARAM_SEED = 1234
CLIP_SEED = 777


@functools.lru_cache(maxsize=None)
def params(label_count):
    p = dscnn.synthetic_params(label_count, PARAM_SEED)
    p.setflags(write=False)
    return p


@functools.lru_cache(maxsize=None)
def clips(n):
    x = dscnn.structured_clips(n, CLIP_SEED)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=2)
def trunk_reference(n):
    """Stages 0..5 (float64) of the first n clips.  The trunk's parameters do not depend on label_count (they are drawn before the dense
    layer's), so one run serves every label_count."""
    stages, _ = dscnn.dscnn_host(clips(n), params(LABEL_COUNTS[0]), "all")
    for s in stages:
        s.setflags(write=False)
    return stages


def logits_reference(n, label_count):
    f = dscnn.fold(params(label_count))
    return trunk_reference(n)[5] @ f["dense_w"].astype(np.float64) + f["dense_b"].astype(np.float64)


def deterministic_clips():
    """All zeros, all 65 535, and single impulses at the four corners and in the last two rows: these show the 4/5 and 1/1 padding of the
    stem and the input rows that only the bottom padding's neighbours read."""
    out, names = [np.zeros((49, 40)), np.full((49, 40), 65535.0)], ["zeros", "full_scale"]
    for r, c in ((0, 0), (0, 39), (48, 0), (48, 39), (47, 17), (48, 22)):
        x = np.zeros((49, 40))
        x[r, c] = 400.0
        out.append(x)
        names.append(f"impulse_{r}_{c}")
    return np.stack(out).astype(np.float32), names


def row24_pair(label_count=7):
    """(clips, params_a, params_b).  The clips are zero outside input row 44, and the two parameter sets differ only in row ky = 0 of the
    stem kernel.  Input row 44 meets ky = 0 at stem-output row 24 alone (2 * 24 - 4 + 0 = 44), so the stem outputs differ in row 24 and
    nowhere else: whatever separates the logits went from row 24 into row 23 through the depthwise taps of the blocks."""
    rng = np.random.default_rng(24)
    x = np.zeros((3, 49, 40), np.float32)
    x[:, 44, :] = np.floor(rng.uniform(100.0, 400.0, (3, 40)))
    a = params(label_count).copy()
    b = a.copy()
    k = dscnn.unpack(b)["conv2d/kernel"]
    k[0] = -2.0 * k[0] + 0.05
    return x, a, b
