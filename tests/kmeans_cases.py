"""Inputs shared by tests/test_kmeans_cpu.py and tests/test_kmeans_gpu.py: blob-plus-noise point sets, built once and left unchanged."""
import numpy as np

SHAPES = [(50, 5, 1024), (20, 3, 1024), (7, 2, 64), (64, 8, 1024)]
NOISE = [0.05, 0.3, 1.0]

_BLOBS = {}


def blobs(n, dim, n_blobs, noise, seed):
    """float32 [n, dim]: n points around n_blobs random centres."""
    key = (n, dim, n_blobs, noise, seed)
    if key not in _BLOBS:
        rng = np.random.default_rng(seed)
        centres = 2.0 * rng.standard_normal((n_blobs, dim))
        x = (centres[rng.integers(0, n_blobs, n)] + noise * rng.standard_normal((n, dim))).astype(np.float32)
        x.setflags(write=False)
        _BLOBS[key] = x
    return _BLOBS[key]


def family_case(i):
    """Case i of 40: (X, n_clusters, seed) over the four shapes, 1-6 blobs, three noise levels, seeds 123..162."""
    n, k, dim = SHAPES[i % 4]
    seed = 123 + i
    return blobs(n, dim, 1 + i % 6, NOISE[(i // 4) % 3], seed), k, seed
