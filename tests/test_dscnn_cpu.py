"""The DS-CNN's host side without a GPU: dscnn_host (the specification the device is held to in tests/test_dscnn_gpu.py) against an
independent float64 restatement with torch.nn.functional on UNFOLDED BatchNorm, the conditions the test inputs must meet (asserted on the
reference alone), and the host plumbing: manifest, import by Keras names, container, C-ABI refusals, predict's input ranks."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(__file__))
import dscnn_cases as cases  # noqa: E402
import util_bundle as ub  # noqa: E402

from multilingual_kws_amd import _lib, dscnn  # noqa: E402


def _torch_reference(spec, params):
    """-> ([stage 0..5], logits), float64, from the raw parameters: convolution, bias, BatchNorm (eps 1e-3), ReLU, layer by layer."""
    t = {k: torch.from_numpy(v.astype(np.float64)) for k, v in dscnn.unpack(params).items()}
    name = lambda kind, i: kind if i == 0 else f"{kind}_{i}"

    def bn(x, i):
        p = name("batch_normalization", i)
        g, b, m, v = (t[f"{p}/{leaf}"].view(1, -1, 1, 1) for leaf in ("gamma", "beta", "moving_mean", "moving_variance"))
        return F.relu((x - m) / torch.sqrt(v + float(np.float32(1e-3))) * g + b)

    x = torch.from_numpy(np.asarray(spec, np.float64))[:, None]                                     # NCHW
    x = F.conv2d(F.pad(x, (1, 1, 4, 5)), t["conv2d/kernel"].permute(3, 2, 0, 1), t["conv2d/bias"], stride=2)
    x = bn(x, 0)
    stages = [x]
    for blk in range(4):
        dw = t[name("depthwise_conv2d", blk) + "/depthwise_kernel"].permute(2, 3, 0, 1)             # [3,3,64,1] -> [64,1,3,3]
        x = bn(F.conv2d(x, dw, t[name("depthwise_conv2d", blk) + "/bias"], padding=1, groups=64), 2 * blk + 1)
        x = bn(F.conv2d(x, t[name("conv2d", blk + 1) + "/kernel"].permute(3, 2, 0, 1), t[name("conv2d", blk + 1) + "/bias"]), 2 * blk + 2)
        stages.append(x)
    pooled = F.avg_pool2d(x, (24, 20)).flatten(1)
    assert pooled.shape[1] == 64
    logits = pooled @ t["dense/kernel"] + t["dense/bias"]
    return [s.permute(0, 2, 3, 1).numpy() for s in stages] + [pooled.numpy()], logits.numpy()


def _rel(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


# The reference above keeps BatchNorm apart and the specification folds it into float32 weights: they differ by the rounding of the folded
# weights (2^-24 relative per weight), far above 1e-12.  So the specification is held to the restatement twice: with exactly folded weights
# (float64, not rounded) within 1e-12, which checks every layer's arithmetic and the folding formula; and fold()'s float32 rounding on its own.
def _fold64(params):
    t = dscnn.unpack(params)
    name = lambda kind, i: kind if i == 0 else f"{kind}_{i}"

    def one(w, bias, i):
        g, b, m, v = (t[f"{name('batch_normalization', i)}/{leaf}"].astype(np.float64) for leaf in ("gamma", "beta", "moving_mean", "moving_variance"))
        scale = g / np.sqrt(v + np.float64(np.float32(1e-3)))
        return w.astype(np.float64) * scale, (bias.astype(np.float64) - m) * scale + b

    out = dict(dw_w=[], dw_b=[], pw_w=[], pw_b=[])
    out["stem_w"], out["stem_b"] = one(t["conv2d/kernel"].reshape(40, 64), t["conv2d/bias"], 0)
    for blk in range(4):
        w, b = one(t[name("depthwise_conv2d", blk) + "/depthwise_kernel"].reshape(9, 64), t[name("depthwise_conv2d", blk) + "/bias"], 2 * blk + 1)
        out["dw_w"].append(w), out["dw_b"].append(b)
        w, b = one(t[name("conv2d", blk + 1) + "/kernel"].reshape(64, 64), t[name("conv2d", blk + 1) + "/bias"], 2 * blk + 2)
        out["pw_w"].append(w), out["pw_b"].append(b)
    out["dense_w"], out["dense_b"] = t["dense/kernel"].astype(np.float64), t["dense/bias"].astype(np.float64)
    return out


@pytest.mark.parametrize("label_count", [7, 12])
def test_host_specification_matches_the_torch_restatement(label_count):
    det, _ = cases.deterministic_clips()
    for spec in (cases.clips(8), det):
        want_stages, want_logits = _torch_reference(spec, cases.params(label_count))
        got_stages, got_logits = dscnn._forward_stages(spec, _fold64(cases.params(label_count)))
        for s in range(6):
            assert got_stages[s].shape == want_stages[s].shape
            assert _rel(got_stages[s], want_stages[s]) < 1e-12, s
        assert _rel(got_logits, want_logits) < 1e-12


def test_fold_is_the_float64_fold_rounded_once():
    exact, got = _fold64(cases.params(7)), dscnn.fold(cases.params(7))
    for key in ("stem_w", "stem_b", "dense_w", "dense_b"):
        assert got[key].dtype == np.float32 and np.array_equal(got[key], exact[key].astype(np.float32)), key
    for key in ("dw_w", "dw_b", "pw_w", "pw_b"):
        for blk in range(4):
            assert got[key][blk].dtype == np.float32 and np.array_equal(got[key][blk], exact[key][blk].astype(np.float32)), (key, blk)
    # and the specification on those float32 weights stays within their rounding of the unfolded network
    want_stages, want_logits = _torch_reference(cases.clips(8), cases.params(7))
    stages, logits = dscnn.dscnn_host(cases.clips(8), cases.params(7), "all")
    assert all(_rel(stages[s], want_stages[s]) < 1e-6 for s in range(6)) and _rel(logits, want_logits) < 1e-5
    assert np.array_equal(dscnn.dscnn_host(cases.clips(8), cases.params(7)), logits)
    assert np.array_equal(dscnn.dscnn_host(cases.clips(8), cases.params(7), 3), stages[3])


@pytest.mark.parametrize("label_count", cases.LABEL_COUNTS)
def test_inputs_keep_the_network_data_dependent(label_count):
    n = 67
    stages = cases.trunk_reference(n)
    logits = cases.logits_reference(n, label_count)
    scale = np.abs(logits).max()
    # every ReLU between 20 % and 80 % alive (the depthwise ReLUs are inside the blocks: taken from a run with a hook)
    alive = []
    dscnn._forward_stages(cases.clips(16), dscnn.fold(cases.params(label_count)), hook=lambda i, y: (alive.append(float((y > 0).mean())), y)[1])
    assert len(alive) == 9 and all(0.2 <= a <= 0.8 for a in alive), alive
    assert all(0.2 <= float((stages[s] > 0).mean()) <= 0.8 for s in range(5))
    assert len(set(logits.argmax(axis=1).tolist())) >= min(3, label_count)
    top2 = np.sort(logits, axis=1)[:, -2:]
    assert float(((top2[:, 1] - top2[:, 0]) < 1e-4 * scale).mean()) <= 0.05
    apart = np.abs(logits[:, None, :] - logits[None, :, :]).max(axis=2) + 10.0 * scale * np.eye(n)
    assert apart.min() > 1e-3 * scale, apart.min() / scale


def test_deterministic_clips_are_told_apart():
    det, names = cases.deterministic_clips()
    logits = dscnn.dscnn_host(det, cases.params(7))
    scale = np.abs(logits[names.index("zeros")]).max()
    apart = np.abs(logits[:, None, :] - logits[None, :, :]).max(axis=2) + 1e30 * np.eye(len(names))
    assert apart.min() > 1e-3 * scale, (apart.min() / scale, names)


def test_row24_reaches_the_logits_through_the_blocks_only():
    x, a, b = cases.row24_pair()
    sa, la = dscnn.dscnn_host(x, a, "all")
    sb, lb = dscnn.dscnn_host(x, b, "all")
    assert np.array_equal(sa[0][:, :24], sb[0][:, :24]) and np.abs(sa[0][:, 24] - sb[0][:, 24]).max() > 1e-2 * np.abs(sa[0]).max()
    assert np.abs(la - lb).max() > 1e-3 * np.abs(la).max()
    # stage-4 row 24 does not reach the pool: the pooled features are the mean of rows 0..23
    assert np.array_equal(sa[5], sa[4][:, :24].mean(axis=(1, 2)))
    assert np.abs(sa[4][:, 24]).max() > 0


def test_manifest_and_parameter_counts():
    assert dscnn.param_count(7) == 24583 and dscnn.param_count(12) == 24908
    for bad in (1, 65, 0, -3):
        with pytest.raises(ValueError):
            dscnn.param_count(bad)
        with pytest.raises(_lib.MkwsError):
            dscnn.manifest(bad)
    man = dscnn.manifest(12)
    assert len(man) == 2 * 5 + 2 * 4 + 4 * 9 + 2
    assert [t["name"] for t in man[:8]] == ["conv2d/kernel", "conv2d/bias", "batch_normalization/gamma", "batch_normalization/beta",
                                            "batch_normalization/moving_mean", "batch_normalization/moving_variance",
                                            "depthwise_conv2d/depthwise_kernel", "depthwise_conv2d/bias"]
    assert [t["name"] for t in man[-8:-2]] == ["conv2d_4/kernel", "conv2d_4/bias"] + [f"batch_normalization_8/{leaf}" for leaf in ("gamma", "beta", "moving_mean", "moving_variance")]
    shapes = {t["name"]: t["shape"] for t in man}
    assert shapes["conv2d/kernel"] == [10, 4, 1, 64] and shapes["depthwise_conv2d_3/depthwise_kernel"] == [3, 3, 64, 1]
    assert shapes["conv2d_2/kernel"] == [1, 1, 64, 64] and shapes["dense/kernel"] == [64, 12] and shapes["dense/bias"] == [12]
    assert man[0]["offset"] == 0 and all(p["offset"] + p["count"] == q["offset"] for p, q in zip(man, man[1:]))
    assert man[-1]["offset"] + man[-1]["count"] == 24908
    assert dscnn.label_count_of(np.zeros(24583, np.float32)) == 7
    with pytest.raises(ValueError):
        dscnn.label_count_of(np.zeros(24584, np.float32))


def _keras_names(params, first):
    """The blob under the names a Keras session gives the layers when its per-kind counters stand at `first`."""
    kinds = {"conv2d": 0, "depthwise_conv2d": 0, "batch_normalization": 0, "dense": 0}
    out = {}
    for name, v in dscnn.unpack(params).items():
        layer, leaf = name.split("/")
        kind, _, num = layer.rpartition("_") if layer.rsplit("_", 1)[-1].isdigit() else (layer, "", "0")
        n = first[kind] + int(num)
        out[(kind if n == 0 else f"{kind}_{n}") + "/" + leaf] = v.copy()
        kinds[kind] += 1
    return out


def test_from_named_tensors_orders_layers_by_suffix_and_refuses_other_networks():
    p = cases.params(12)
    named = _keras_names(p, dict(conv2d=7, depthwise_conv2d=0, batch_normalization=98, dense=3))
    assert "conv2d_7/kernel" in named and "batch_normalization_106/gamma" in named and "dense_3/bias" in named and "depthwise_conv2d/bias" in named
    keys = list(named)
    np.random.default_rng(0).shuffle(keys)
    assert np.array_equal(dscnn.from_named_tensors({k: named[k] for k in keys}), p)
    assert np.array_equal(dscnn.from_named_tensors({k + ":0": v for k, v in named.items()}), p)
    # suffixes 9, 10, 11 must order numerically, not as strings
    named = _keras_names(p, dict(conv2d=8, depthwise_conv2d=9, batch_normalization=2, dense=0))
    assert np.array_equal(dscnn.from_named_tensors(named), p)

    plain = _keras_names(p, dict(conv2d=0, depthwise_conv2d=0, batch_normalization=0, dense=0))
    def without(*names):
        return {k: v for k, v in plain.items() if k not in names}
    for bad in (without("conv2d_4/kernel", "conv2d_4/bias"),                                    # a layer short
                without("batch_normalization_3/moving_mean"),                                   # a variable short
                dict(plain, **{"stem_conv/kernel": np.zeros((3, 3, 1, 32), np.float32)}),       # another network's layer
                dict(plain, **{"dense_1/kernel": np.zeros((64, 12), np.float32), "dense_1/bias": np.zeros(12, np.float32)}),
                dict(plain, **{"conv2d_2/kernel": np.zeros((3, 3, 64, 64), np.float32)}),       # wrong shape
                dict(plain, **{"conv2d/kernel": np.zeros((10, 4, 1, 32), np.float32)}),
                dict(plain, **{"dense/kernel": np.zeros((64, 65), np.float32), "dense/bias": np.zeros(65, np.float32)}),
                dict(plain, **{"conv2d_1/gamma": np.zeros(64, np.float32)})):
        with pytest.raises(ValueError):
            dscnn.from_named_tensors(bad)


def test_load_keras_reads_a_savedmodel_whose_layer_numbers_do_not_start_at_zero(tmp_path):
    p = cases.params(7)
    named = _keras_names(p, dict(conv2d=5, depthwise_conv2d=4, batch_normalization=9, dense=1))
    layers = []
    for name in named:                                      # (layer order as the blob's: the names alone must decide)
        layer, leaf = name.split("/")
        if not layers or layers[-1][0] != layer:
            layers.append((layer, []))
        layers[-1][1].append(leaf)
    graph, keys = ub.keras_object_graph(layers)
    os.makedirs(tmp_path / "m" / "variables")
    tensors = {keys[name]: v for name, v in named.items()}
    tensors["optimizer/iter/.ATTRIBUTES/VARIABLE_VALUE"] = np.zeros((), np.int64)
    ub.write_bundle(str(tmp_path / "m" / "variables" / "variables"), tensors, graph)
    assert np.array_equal(dscnn.load_keras(str(tmp_path / "m")), p)


def test_save_load_round_trip(tmp_path):
    p = cases.params(7)
    dscnn.save(str(tmp_path / "m"), p)
    assert sorted(os.listdir(tmp_path / "m")) == ["manifest.json", "weights.bin"]
    back = dscnn.load(str(tmp_path / "m"))
    assert back.dtype == np.float32 and np.array_equal(back, p)
    (tmp_path / "m" / "weights.bin").write_bytes(p[:-1].tobytes())
    with pytest.raises(ValueError):
        dscnn.load(str(tmp_path / "m"))
    with pytest.raises(ValueError):
        dscnn.save(str(tmp_path / "n"), p[:-1])


def test_create_refuses_bad_weights_before_it_looks_for_a_device():
    L = _lib.lib()
    h = ctypes.c_void_p()
    p = np.ascontiguousarray(cases.params(7))
    BAD_WEIGHTS, NO_DEVICE = -6, -3
    assert L.mkws_dscnn_create(p.ctypes.data, p.shape[0] - 1, 7, 4, ctypes.byref(h)) == BAD_WEIGHTS
    assert L.mkws_dscnn_create(p.ctypes.data, p.shape[0], 8, 4, ctypes.byref(h)) == BAD_WEIGHTS
    assert L.mkws_dscnn_create(p.ctypes.data, 24128 + 65, 1, 4, ctypes.byref(h)) == BAD_WEIGHTS
    assert L.mkws_dscnn_create(p.ctypes.data, 24128 + 65 * 65, 65, 4, ctypes.byref(h)) == BAD_WEIGHTS
    nan = p.copy()
    nan[100] = np.nan
    assert L.mkws_dscnn_create(nan.ctypes.data, nan.shape[0], 7, 4, ctypes.byref(h)) == BAD_WEIGHTS
    assert h.value is None
    if not torch.cuda.is_available():
        assert L.mkws_dscnn_create(p.ctypes.data, p.shape[0], 7, 4, ctypes.byref(h)) == NO_DEVICE
        assert b"no HIP device" in L.mkws_last_error()
        with pytest.raises(_lib.MkwsError) as e:
            dscnn.DSCNN(p)
        assert e.value.code == NO_DEVICE
    assert L.mkws_dscnn_param_count(7) == 24583 and L.mkws_dscnn_param_count(1) == 0 and L.mkws_dscnn_param_count(65) == 0


def test_predict_takes_both_input_ranks_and_batches(monkeypatch):
    """The device call is replaced: predict's job is the ranks, the batching by max_batch and the NumPy result."""
    m = dscnn.DSCNN.__new__(dscnn.DSCNN)
    m.h, m.max_batch, m.label_count, seen = None, 3, 7, []

    def forward(spec):
        seen.append(tuple(spec.shape))
        return torch.from_numpy(dscnn.softmax_host(np.asarray(spec, np.float64).sum(axis=(1, 2))[:, None] * np.arange(7.0) * 1e-5).astype(np.float32))

    monkeypatch.setattr(m, "forward", forward, raising=False)
    x = cases.clips(8)
    a, b = m.predict(x), m.predict(x[..., None])
    assert seen == [(3, 49, 40), (3, 49, 40), (2, 49, 40)] * 2
    assert a.shape == (8, 7) and a.dtype == np.float32 and np.array_equal(a, b) and isinstance(a, np.ndarray)
    assert m.predict(x[:0]).shape == (0, 7)
    for bad in (x[0], x[:, :48], x[..., None, None]):
        with pytest.raises(ValueError):
            m.predict(bad)
