"""The weight sets and clips of tests/util_embed_blobs.py, without a device: what makes them telling, and that the
REFERENCE ALONE is well inside the bounds tests/test_embed_weights_gpu.py holds the kernels to.

  * the deltas are there: negative and small gammas are counted, the epsilon-ruled channels have a moving variance below epsilon, every gate
    tap of wide_gates reaches both saturated tails, the normalised stem differs from the mean-0 / variance-1 stem on border and interior pixels;
  * no (set, clip, tap) of the float64 oracle is degenerate;
  * forward condition: on every (set, clip, tap) the float32 oracle is within a THIRD of REL_TOL = 1e-4 of the float64 one, relative to that
    clip's own largest value.  A set that misses it gets another seed (util_embed_blobs.SEEDS), never another cap;
  * training-step condition (the inputs of test_training_mode_gradients_match_the_oracle, on `everything` and `normalized`): the float32
    TrainableEmbeddingOracle within a TENTH of that test's gradient bound of the float64 one, the training-mode embedding within 1e-5, and no
    float64 pre-activation of dense / dense_1 within 1e-5 x the layer's largest of zero (a ReLU cell float32 cannot place would move a bias
    gradient by more than the bound; the clip seed util_embed_blobs.TRAIN_SEED is chosen for this).
Every measured figure is printed before it is asserted."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import util_embed_blobs as ub  # noqa: E402
from oracle.efficientnet_oracle import split_blob  # noqa: E402

torch = pytest.importorskip("torch")

REL_TOL = 1e-4                    # tests/test_embedding_gpu.py
FORWARD_CAP = REL_TOL / 3
BN_EPS = 1e-3


def _seed_blob():
    from multilingual_kws_amd import weights
    return weights.synthetic_blob()


def _changed(name):
    """Tensor names in which blob(name) differs from the seed-1234 blob."""
    a, b = split_blob(_seed_blob()), split_blob(ub.blob(name))
    return {k for k in a if not np.array_equal(a[k], b[k])}


def _is_stat(k):
    return k.endswith(("/moving_mean", "/moving_variance"))


def _forward_condition(name):
    """No tap degenerate; float32 oracle within FORWARD_CAP of the float64 one on every (clip, tap) and on the embedding."""
    emb, taps = ub.reference(name)
    emb32, taps32 = ub.forward_reference(ub.blob(name), torch.float32)
    taps, taps32 = dict(taps, embedding=emb), dict(taps32, embedding=emb32)
    assert len(taps) == 70
    worst = (0.0, None, None)
    for tap, ref in taps.items():
        for c, clip in enumerate(ub.CLIP_NAMES):
            top = float(np.abs(ref[c]).max())
            assert np.isfinite(ref[c]).all() and top > 0.0, (name, clip, tap)
            worst = max(worst, (float(np.abs(taps32[tap][c] - ref[c]).max()) / top, tap, clip))
    print("%s: max |fp32 oracle - fp64 oracle| / max |fp64 tap of the clip| = %.3g (%s, %s); cap %.3g" % ((name,) + worst + (FORWARD_CAP,)))
    assert worst[0] <= FORWARD_CAP, (name, worst)


def test_clips():
    x = ub.clips()
    assert x.shape == (8, 49, 40) and x.dtype == np.float32 and len(ub.CLIP_NAMES) == 8 and not x.flags.writeable
    k = x / ub.GRID
    assert np.array_equal(k, np.round(k)) and k.min() == 0 and k.max() == ub.FULL_SCALE                  # on the value grid
    c = {n: k[i] for i, n in enumerate(ub.CLIP_NAMES)}
    for n in ("noise0", "noise1", "noise2"):
        assert (c[n] > 0).mean() > 0.99 and len(np.unique(c[n])) > 500
    assert not c["silent"].any()
    assert c["loud"].min() >= 500 and c["loud"].max() <= 670
    assert c["corners_a"][0, 0] == 670 and c["corners_a"][48, 39] == 670 and np.count_nonzero(c["corners_a"]) == 2
    assert c["corners_b"][0, 39] == 670 and c["corners_b"][48, 0] == 670 and c["corners_b"][24, 20] == 335 and np.count_nonzero(c["corners_b"]) == 3
    assert 0.77 < (c["sparse"] == 0).mean() < 0.83
    # spectrogram values / 255 lie in [0, 0.103]: a normalised background pixel is -1.33
    assert x.max() / 255 < 0.103 and abs((0 - ub.NORM_MEAN) / np.sqrt(ub.NORM_VARIANCE) + 4 / 3) < 1e-6


def test_blobs_are_seeded_and_read_only():
    for name in ub.SETS:
        b = ub.blob(name)
        assert b.dtype == np.float32 and b.shape == _seed_blob().shape and not b.flags.writeable and np.isfinite(b).all()
        assert ub.blob(name) is b
        w = split_blob(b)
        for k, v in w.items():
            if _is_stat(k):
                assert np.array_equal(v * 4096, np.round(v * 4096)), k                                   # the 2^-12 grid
                if k.endswith("variance"):
                    assert v.min() >= 1 / 4096, k
    assert np.array_equal(ub.blob.__wrapped__("everything"), ub.blob("everything"))          # built again from its seeds: the same bits


def test_normalized():
    name = "normalized"
    w = split_blob(ub.blob(name))
    assert w["normalization/mean"][0] == np.float32(0.04) and w["normalization/variance"][0] == np.float32(9e-4)
    assert {k for k in _changed(name) if not _is_stat(k)} == {"normalization/mean", "normalization/variance"}         # nothing else changes
    # the stem of the same weights with mean 0 / variance 1: different on border pixels as well as interior ones
    assert ub.twin(name)[2:].tobytes() == ub.blob(name)[2:].tobytes()
    stem = ub.reference(name)[1]["stem"].reshape(8, 25, 20, 32)
    other = ub.forward_reference(ub.twin(name))[1]["stem"].reshape(8, 25, 20, 32)
    d = np.abs(stem - other).max(axis=3)                               # [clip, row, column]
    border = np.ones((25, 20), bool)
    border[1:-1, :-1] = False                                           # correct_pad(49, 40, 3): padded rows above and below, a padded column right
    scale = np.abs(stem).max()
    print("normalized: stem differs from the mean-0 twin by at least %.3g of its largest value on border pixels, %.3g on interior ones"
          % (d[:, border].min() / scale, d[:, ~border].min() / scale))
    assert d[:, border].min() > 1e-3 * scale and d[:, ~border].min() > 1e-3 * scale
    # the order matters on the border: normalising the padded pixel too (pad, then normalise) gives another stem there and the same one inside
    o = ub._oracle(ub.blob(name), torch.float64)
    x = torch.from_numpy(np.array(ub.clips())).to(torch.float64)[:, None]
    with torch.no_grad():
        padded_first = o.preprocess(torch.nn.functional.pad(x, (0, 1, 1, 1)))
        wrong = o._swish(o._bn(o._conv(padded_first, "stem_conv/kernel", stride=2), "stem_bn")).permute(0, 2, 3, 1).numpy()
    dw = np.abs(wrong - stem).max(axis=3)
    assert dw[:, ~border].max() < 1e-12 * scale and dw[:, border].max() > 1e-2 * scale
    _forward_condition(name)


def test_signed_gamma():
    name = "signed_gamma"
    w = split_blob(ub.blob(name))
    assert {k.split("/")[-1] for k in _changed(name) if not _is_stat(k)} == {"gamma", "beta"}
    g = np.concatenate([v for k, v in w.items() if k.endswith("/gamma")])
    b = np.concatenate([v for k, v in w.items() if k.endswith("/beta")])
    print("signed_gamma: %d gammas, %.3f negative, %.3f below 0.2 in magnitude, |gamma| in [%.3g, %.3g]; beta sd %.3f"
          % (g.size, (g < 0).mean(), (np.abs(g) < 0.2).mean(), np.abs(g).min(), np.abs(g).max(), b.std()))
    assert 0.30 < (g < 0).mean() < 0.37 and 0.05 <= np.abs(g).min() < 0.051 and 2.99 < np.abs(g).max() <= 3.0
    assert 0.30 < (np.abs(g) < 0.2).mean() < 0.38                     # log-uniform: ln(0.2 / 0.05) / ln(3 / 0.05) = 0.339
    assert 0.97 < b.std() < 1.03
    for k, v in w.items():                                              # every BatchNorm has negative and small gammas of its own
        if k.endswith("/gamma"):
            assert (v < 0).any() and (v > 0).any() and (np.abs(v) < 0.2).any(), k
    _forward_condition(name)


def test_eps_ruled():
    name = "eps_ruled"
    w = split_blob(ub.blob(name))
    seed = split_blob(_seed_blob())
    touched = [k for k in w if k.endswith(ub.EPS_RULED_KERNELS)]
    assert len(touched) == 15 + 16 + 16 + 1 and {k for k in _changed(name) if not _is_stat(k)} == set(touched)
    worst = 1.0
    for k in touched:
        axis = 2 if k.endswith("depthwise_kernel") else 3
        ratio = np.abs(w[k]).sum(axis=tuple(a for a in range(4) if a != axis)) / np.abs(seed[k]).sum(axis=tuple(a for a in range(4) if a != axis))
        scaled = np.isclose(ratio, 2.0 ** -6)
        assert scaled.sum() == scaled.size // 8 and np.isclose(ratio[~scaled], 1.0).all(), k
        var = w[ub.bn_of_kernel(k) + "/moving_variance"]
        worst = min(worst, float((var < BN_EPS).mean()))
        assert (var < BN_EPS).mean() >= 0.1, (k, float((var < BN_EPS).mean()))
        assert (var[scaled] < BN_EPS).all(), k                          # ... and they are the scaled ones
    print("eps_ruled: smallest share of a touched BatchNorm's channels with moving_variance < 1e-3: %.4f" % worst)
    _forward_condition(name)


def test_wide_gates():
    name = "wide_gates"
    w = split_blob(ub.blob(name))
    assert {k for k in _changed(name) if not _is_stat(k)} == {k for k in w if k.endswith("/bias")}
    for leaf, sd in (("_se_expand/bias", 2.0), ("_se_reduce/bias", 0.5)):
        v = np.concatenate([x for k, x in w.items() if k.endswith(leaf)])
        assert 0.9 * sd < v.std() < 1.1 * sd, (leaf, v.std())
    for k in ("dense/bias", "dense_1/bias", "dense_2/bias"):
        assert 0.27 < w[k].std() < 0.33, k
    gates = {k: v for k, v in ub.reference(name)[1].items() if k.endswith("_gate")}
    assert len(gates) == 16
    for k, v in gates.items():
        print("wide_gates: %s over the eight clips in [%.3g, %.4f]" % (k, v.min(), v.max()))
        assert v.min() < 0.02 and v.max() > 0.98, (k, v.min(), v.max())
    _forward_condition(name)


def test_everything():
    name = "everything"
    w = split_blob(ub.blob(name))
    assert w["normalization/mean"][0] == np.float32(0.04) and w["normalization/variance"][0] == np.float32(9e-4)
    g = np.concatenate([v for k, v in w.items() if k.endswith("/gamma")])
    assert 0.30 < (g < 0).mean() < 0.37 and (np.abs(g) < 0.2).mean() > 0.30
    below = {k: float((w[ub.bn_of_kernel(k) + "/moving_variance"] < BN_EPS).mean()) for k in w if k.endswith(ub.EPS_RULED_KERNELS)}
    gates = {k: v for k, v in ub.reference(name)[1].items() if k.endswith("_gate")}
    print("everything: %.3f of the gammas negative; mean share of epsilon-ruled channels %.3f (least %.3f); gates in [%.3g, %.4f]"
          % ((g < 0).mean(), np.mean(list(below.values())), min(below.values()), min(v.min() for v in gates.values()), max(v.max() for v in gates.values())))
    # (with gammas up to 3 in front of it a scaled channel's variance does not always reach the floor: most do)
    assert np.mean(list(below.values())) > 0.1 and min(below.values()) > 0.05
    assert all(v.min() < 0.02 and v.max() > 0.98 for v in gates.values())
    assert np.std(w["block3a_se_expand/bias"]) > 1.5 and np.std(w["dense_1/bias"]) > 0.27
    _forward_condition(name)


def test_seed_1234_blob_on_these_clips():
    """The gentle blob itself on the eight clips: the condition is one the inputs can meet, not one the seeds were bent to."""
    emb, taps = ub.forward_reference(_seed_blob())
    emb32, taps32 = ub.forward_reference(_seed_blob(), torch.float32)
    worst = max((float(np.abs(taps32[t][c] - taps[t][c]).max() / np.abs(taps[t][c]).max()), t, ub.CLIP_NAMES[c]) for t in taps for c in range(8))
    print("seed-1234 blob: max |fp32 oracle - fp64 oracle| / max |fp64 tap of the clip| = %.3g (%s, %s)" % worst)
    assert worst[0] <= FORWARD_CAP


@pytest.mark.parametrize("name", ub.TRAIN_SETS)
def test_training_step_condition(name):
    spec, proj, masks = ub.train_inputs()
    assert spec.shape == (6, 49, 40) and proj.shape == (1024,) and sorted(masks) == ["2b", "4c", "6d"] and all(m.shape == (6,) for m in masks.values())
    r64 = ub.train_reference64(name)
    r32 = ub.train_reference(ub.blob(name), torch.float32)
    # no ReLU cell that float32 cannot place
    for layer, pre in r64["pre"].items():
        assert pre.shape == (6, 2048)
        nearest = float(np.abs(pre).min() / np.abs(pre).max())
        print("%s: %s pre-activation nearest to zero: %.3g of the layer's largest (must be above 1e-5)" % (name, layer, nearest))
        assert nearest > 1e-5, (name, layer, nearest)
        assert np.array_equal(r32["pre"][layer] > 0, pre > 0), (name, layer)
    # training-mode embedding
    e = float(np.abs(r32["emb"] - r64["emb"]).max() / np.abs(r64["emb"]).max())
    print("%s: training-mode embedding, fp32 oracle against fp64: %.3g (cap 1e-5)" % (name, e))
    assert e <= 1e-5, (name, e)
    # every trainable tensor's gradient, in the metric of test_training_mode_gradients_match_the_oracle: a tenth of its bound
    gmax = max(float(np.abs(g).max()) for g in r64["grads"].values())
    assert len(r64["grads"]) == len(r64["trainable"]) and all(g is not None for g in r64["grads"].values())
    share = {k: float(np.abs(r32["grads"][k] - g).max()) / ub.gradient_bound(g, gmax) for k, g in r64["grads"].items()}
    k = max(share, key=share.get)
    print("%s: largest share of the gradient bound the fp32 oracle uses: %.3g (%s), i.e. %.3g against the bound 1e-3; gmax %.3g"
          % (name, share[k], k, 1e-3 * share[k], gmax))
    assert share[k] <= 0.1, (name, k, share[k])
    # updated moving statistics
    m = max(float(np.abs(r32["moving"][k] - v).max() / np.abs(v).max()) for k, v in r64["moving"].items())
    print("%s: new moving statistics, fp32 oracle against fp64: %.3g (the device is held to 1e-5)" % (name, m))
    assert m <= 1e-6


def test_normalization_reaches_the_stem_gradient():
    """What tests/test_embed_weights_gpu.py asserts of the device holds of the reference: the stem_conv/kernel gradient of `normalized` differs
    from that of its mean-0 / variance-1 twin by far more than the bound."""
    g = ub.train_reference64("normalized")["grads"]
    t = ub.train_reference64("normalized", True)["grads"]
    gmax = max(float(np.abs(v).max()) for v in g.values())
    d = float(np.abs(g["stem_conv/kernel"] - t["stem_conv/kernel"]).max())
    print("normalized: stem_conv/kernel gradient differs from the twin's by %.3g, bound %.3g" % (d, ub.gradient_bound(g["stem_conv/kernel"], gmax)))
    assert d > 100 * ub.gradient_bound(g["stem_conv/kernel"], gmax)
