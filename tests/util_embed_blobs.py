"""Named weight sets for the embedding network, each a stated delta of weights.synthetic_blob() (seed 1234), and eight named clips
(DESIGN.md section 34).  Pure NumPy plus the project's float64 oracle: no device, and the product package stays free of a host forward pass.

The seed-1234 blob is gentle on purpose (tools/calibrate_synthetic_bn.py bounds every channel's gain): normalization mean 0 / variance 1,
every gamma in [0.5, 1.5], every moving variance far above epsilon, every bias N(0, 0.02^2).  A kernel that drops a term which is zero there, or
mishandles a sign that is positive there, passes every test that starts from it.  The sets:

  normalized    normalization/mean = 0.04, normalization/variance = 9e-4: spectrogram values / 255 lie in [0, 0.103], so a normalised
                background pixel is -1.33 and a zero-padded one 0 (Keras: normalise, THEN pad).  Nothing else changes.
  signed_gamma  every gamma log-uniform in [0.05, 3] with a third of them negative; every beta N(0, 1).
  eps_ruled     an eighth of the output channels of every expand, depthwise, project and top kernel scaled by 2^-6: their calibrated variance
                falls by 2^-12 to the floor of the grid, and epsilon = 1e-3 alone sets their gain.
  wide_gates    *_se_expand/bias N(0, 2^2), *_se_reduce/bias N(0, 0.5^2), dense biases N(0, 0.3^2): gates reach both saturated tails.
  everything    all of the above together.

A set is made from synthetic_blob() by (1) its delta, (2) every moving_mean / moving_variance set from float64 activations of 16 calibration
clips, walking the ORACLE'S OWN layers (a subclass whose _bn measures before it normalises: the recipe cannot drift from what it calibrates),
(3) the seeded perturbation mean += 0.1 sd N(0,1), var *= U(0.7, 1.4), (4) quantisation to the 2^-12 grid as tools/calibrate_synthetic_bn.py
does -- with a variance floor of one grid step, 2.4e-4, which is BELOW epsilon (that tool's "no near-dead channels" bound is what is left out).
Random draws come from np.random.default_rng([seed of the set, stream]); tests/test_embed_blobs_cpu.py holds what the seeds were chosen for."""
import functools
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from oracle.efficientnet_oracle import EmbeddingOracle, split_blob, tensor_list  # noqa: E402

SETS = ("normalized", "signed_gamma", "eps_ruled", "wide_gates", "everything")
# per-name seeds.  Chosen (tests/test_embed_blobs_cpu.py) so that every gate tap of wide_gates reaches both tails and the float32 oracle keeps
# the conditions on the reference; a set that misses a condition gets another seed, never another cap.
SEEDS = {"normalized": 103, "signed_gamma": 102, "eps_ruled": 103, "wide_gates": 104, "everything": 110}
_DELTA, _CALIB_CLIPS, _PERTURB = 0, 1, 2            # random streams of a set

GRID = np.float32(10 / 256)                          # spectrogram value grid: k * 10/256, k in [0, 670]
FULL_SCALE = 670
CLIP_NAMES = ("noise0", "noise1", "noise2", "silent", "loud", "corners_a", "corners_b", "sparse")
NOISE = (0, 1, 2)
CLIP_SEED = 8
NORM_MEAN, NORM_VARIANCE = 0.04, 9e-4
EPS_RULED_SCALE = 2.0 ** -6
EPS_RULED_KERNELS = ("_expand_conv/kernel", "_dwconv/depthwise_kernel", "_project_conv/kernel", "top_conv/kernel")

# the inputs of tests/test_train_gpu.py::test_training_mode_gradients_match_the_oracle; the clip seed is the one at which no float64
# pre-activation of dense / dense_1 lies within 1e-5 of zero on either set the training tests use (tests/test_embed_blobs_cpu.py)
TRAIN_SETS = ("everything", "normalized")
TRAIN_SEED = 26
TRAIN_MASKS = {"2b": np.array([1, 1, 0, 1, 1, 1], bool), "4c": np.array([1, 0, 1, 1, 0, 1], bool), "6d": np.array([0, 1, 1, 1, 1, 1], bool)}


def _readonly(a):
    a.setflags(write=False)
    return a


def _oracle(blob, dtype):
    return EmbeddingOracle(np.array(blob), dtype=dtype)         # (a writable copy: torch.from_numpy warns on a read-only array)


# -- deltas -------------------------------------------------------------------------------------------------------------------------------
def _delta_normalized(w, rng):
    w["normalization/mean"][...] = NORM_MEAN
    w["normalization/variance"][...] = NORM_VARIANCE


def _delta_signed_gamma(w, rng):
    for name in w:
        if name.endswith("/gamma"):
            mag = np.exp(rng.uniform(np.log(0.05), np.log(3.0), w[name].shape))
            w[name][...] = np.where(rng.uniform(0, 1, w[name].shape) < 1 / 3, -mag, mag)
        elif name.endswith("/beta"):
            w[name][...] = rng.standard_normal(w[name].shape)


def eps_ruled_channels(w, rng):
    """{kernel name: sorted output channels scaled by 2^-6}: a random eighth of each."""
    out = {}
    for name in w:
        if name.endswith(EPS_RULED_KERNELS):
            c = w[name].shape[2] if name.endswith("depthwise_kernel") else w[name].shape[3]
            out[name] = np.sort(rng.choice(c, size=c // 8, replace=False))
    return out


def _delta_eps_ruled(w, rng):
    for name, ch in eps_ruled_channels(w, rng).items():
        if name.endswith("depthwise_kernel"):
            w[name][:, :, ch, :] *= EPS_RULED_SCALE
        else:
            w[name][:, :, :, ch] *= EPS_RULED_SCALE


def _delta_wide_gates(w, rng):
    for name in w:
        if name.endswith("_se_expand/bias"):
            w[name][...] = 2.0 * rng.standard_normal(w[name].shape)
        elif name.endswith("_se_reduce/bias"):
            w[name][...] = 0.5 * rng.standard_normal(w[name].shape)
        elif name in ("dense/bias", "dense_1/bias", "dense_2/bias"):
            w[name][...] = 0.3 * rng.standard_normal(w[name].shape)


_DELTAS = {"normalized": (_delta_normalized,), "signed_gamma": (_delta_signed_gamma,), "eps_ruled": (_delta_eps_ruled,),
           "wide_gates": (_delta_wide_gates,), "everything": (_delta_signed_gamma, _delta_eps_ruled, _delta_wide_gates, _delta_normalized)}


def bn_of_kernel(name):
    """The BatchNorm prefix behind a conv kernel: block2a_dwconv/depthwise_kernel -> block2a_bn, top_conv/kernel -> top_bn, ..."""
    layer = name.split("/")[0]
    return layer.replace("_dwconv", "_bn") if layer.endswith("_dwconv") else layer.replace("_conv", "_bn")


# -- calibration --------------------------------------------------------------------------------------------------------------------------
class _Calibrator(EmbeddingOracle):
    """The float64 oracle with a _bn that first SETS the layer's moving statistics from the activations in front of it (perturbed,
    quantised), then normalises with them as the oracle does: every other layer is the oracle's own."""

    def __init__(self, blob, rng):
        super().__init__(blob, dtype=torch.float64)
        self.rng, self.stats = rng, {}

    def _bn(self, x, p):
        c = x.shape[1]
        mean = x.mean(dim=(0, 2, 3)).numpy()
        var = x.var(dim=(0, 2, 3), unbiased=False).numpy()
        mean = mean + 0.1 * np.sqrt(var) * self.rng.standard_normal(c)
        var = var * self.rng.uniform(0.7, 1.4, c)
        mean = np.round(mean * 4096.0) / 4096.0
        var = np.maximum(np.round(var * 4096.0), 1.0) / 4096.0            # floor: one grid step, 2.4e-4 < epsilon
        for leaf, v in (("/moving_mean", mean), ("/moving_variance", var)):
            self.stats[p + leaf] = v
            self.w[p + leaf] = torch.from_numpy(v)
        return super()._bn(x, p)


def calibration_clips(rng):
    """16 clips of noise on the value grid, the last four 70 % sparse."""
    x = rng.integers(0, FULL_SCALE, size=(16, 49, 40)).astype(np.float64)
    x[12:] *= rng.uniform(0, 1, (4, 49, 40)) > 0.7
    return x * float(GRID)


@functools.lru_cache(maxsize=None)
def blob(name):
    """float32 weights of the set `name`, built once, read-only."""
    from multilingual_kws_amd import weights
    seed = SEEDS[name]
    b = weights.synthetic_blob().copy()
    w = split_blob(b)                                   # views into b
    rng = np.random.default_rng([seed, _DELTA])
    for delta in _DELTAS[name]:
        delta(w, rng)
    cal = _Calibrator(b, np.random.default_rng([seed, _PERTURB]))
    with torch.no_grad():
        cal.forward(calibration_clips(np.random.default_rng([seed, _CALIB_CLIPS])))
    n_bn = sum(1 for n, _ in tensor_list() if n.endswith("/moving_mean"))
    assert len(cal.stats) == 2 * n_bn
    for k, v in cal.stats.items():
        w[k][...] = v
    assert np.isfinite(b).all()
    return _readonly(b)


@functools.lru_cache(maxsize=None)
def twin(name):
    """The very weights of blob(name) with normalization mean 0 / variance 1 (nothing recalibrated): what a stem that drops the
    normalization computes."""
    b = blob(name).copy()
    w = split_blob(b)
    w["normalization/mean"][...] = 0.0
    w["normalization/variance"][...] = 1.0
    return _readonly(b)


# -- clips and references -----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def clips():
    """float32 [8, 49, 40], rows named by CLIP_NAMES, on the value grid, read-only."""
    rng = np.random.default_rng(CLIP_SEED)
    k = np.zeros((8, 49, 40), np.int64)
    k[0:3] = rng.integers(0, FULL_SCALE, size=(3, 49, 40))
    k[4] = rng.integers(500, FULL_SCALE + 1, size=(49, 40))
    k[5, 0, 0] = k[5, 48, 39] = FULL_SCALE
    k[6, 0, 39] = k[6, 48, 0] = FULL_SCALE
    k[6, 24, 20] = FULL_SCALE // 2
    k[7] = rng.integers(0, FULL_SCALE, size=(49, 40)) * (rng.uniform(0, 1, (49, 40)) >= 0.8)
    return _readonly(k.astype(np.float32) * GRID)


def forward_reference(b, dtype=torch.float64):
    """(embedding [8, 1024], {tap: [8, -1]}) of the eight clips from the oracle in `dtype`, as float64 arrays."""
    taps = {}
    with torch.no_grad():
        emb = _oracle(b, dtype).forward(np.array(clips()), taps).numpy().astype(np.float64)
    return emb, {k: v.reshape(8, -1).astype(np.float64) for k, v in taps.items()}


@functools.lru_cache(maxsize=None)
def reference(name):
    """The float64 oracle's embedding and 69 taps of the eight clips, from the very blob a handle of the set is created from.  Shared:
    leave it unchanged."""
    emb, taps = forward_reference(blob(name))
    assert len(taps) == 69
    return _readonly(emb), {k: _readonly(v) for k, v in taps.items()}


@functools.lru_cache(maxsize=None)
def train_inputs():
    """(spec [6, 49, 40] float32, proj [1024] float64, drop masks): test_training_mode_gradients_match_the_oracle's, at TRAIN_SEED."""
    rng = np.random.default_rng(TRAIN_SEED)
    spec = rng.integers(0, 670, size=(6, 49, 40)).astype(np.float32) * GRID
    proj = rng.standard_normal(1024)
    return _readonly(spec), _readonly(proj), TRAIN_MASKS


def train_reference(b, dtype=torch.float64):
    """One training-mode step of TrainableEmbeddingOracle in `dtype` on train_inputs(): {"emb", "grads" (trainable tensors), "moving" (the
    updated moving statistics), "pre" (the pre-activations of dense and dense_1)}, all float64 arrays."""
    from oracle.efficientnet_train_oracle import TrainableEmbeddingOracle
    spec, proj, masks = train_inputs()
    o = TrainableEmbeddingOracle(np.array(b), dtype=dtype)
    o.zero_grad()
    pre, relu = [], torch.relu

    def spy(t):                                         # the oracle's only two ReLUs are those of dense and dense_1
        pre.append(t.detach().numpy().astype(np.float64))
        return relu(t)

    torch.relu = spy
    try:
        emb = o.forward(np.array(spec), training=True, drop_masks={k: torch.tensor(v) for k, v in masks.items()})
    finally:
        torch.relu = relu
    assert len(pre) == 2
    (emb @ torch.from_numpy(np.array(proj)).to(dtype)).sum().backward()
    return {"emb": emb.detach().numpy().astype(np.float64), "grads": {k: g.astype(np.float64) for k, g in o.grads().items()},
            "moving": {k: v.detach().numpy().astype(np.float64) for k, v in o.new_moving.items()}, "pre": {"dense": pre[0], "dense_1": pre[1]},
            "trainable": list(o.trainable)}


@functools.lru_cache(maxsize=None)
def train_reference64(name, twin_of=False):
    """The float64 training step of blob(name) (or of its mean-0 / variance-1 twin), computed once."""
    return train_reference(twin(name) if twin_of else blob(name))


def gradient_bound(g, gmax):
    """test_training_mode_gradients_match_the_oracle's bound on a tensor's gradient error: 1e-3 of its largest, floor 1e-6 of the network's."""
    return 1e-3 * float(np.abs(g).max()) + 1e-6 * gmax
