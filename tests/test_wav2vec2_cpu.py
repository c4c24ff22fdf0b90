"""The wav2vec 2.0 baseline without a device: the specification (wav2vec2.reference_forward) against Hugging Face's own float64 forward
(the golden files, and the live model where transformers is importable), the manifest, the loaders, every refusal of
mkws_w2v2_create and of the wrapper, the seeded weights and the reference's draws.

Bound: the float64 restatement and Hugging Face's float64 forward are the same sums in other orders; 1e-12 * max |y| is four orders
above what was seen (2e-15) and five below float32."""
import ctypes
import hashlib
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import wav2vec2_cases as cases  # noqa: E402

from multilingual_kws_amd import _lib, dataperf_wav2vec2, wav2vec2  # noqa: E402

TOL64 = 1e-12
BASE = wav2vec2.Config()


@pytest.mark.parametrize("n", cases.GOLDEN_LENGTHS)
@pytest.mark.parametrize("name", sorted(cases.CONFIGS))
def test_reference_forward_reproduces_the_golden_files(name, n):
    g, c = cases.golden(name), cases.golden_case(name, n)
    T = cases.FRAMES[n]
    assert g[f"{n}_hidden"].shape == (2, T, cases.CONFIGS[name].hidden_size) and np.isfinite(g[f"{n}_hidden"]).all()
    assert cases.rel_err(c.hidden, g[f"{n}_hidden"]) <= TOL64
    assert cases.rel_err(c.embed, g[f"{n}_pooled"]) <= TOL64
    r = wav2vec2.reference_forward(cases.CONFIGS[name], cases.params(name), np.array(g[f"{n}_audio"]))
    assert r.taps is None and cases.rel_err(r.extract_features.numpy(), g[f"{n}_features"]) <= TOL64
    assert np.array_equal(g[f"{n}_pooled"], g[f"{n}_hidden"].max(axis=1))


def test_reference_forward_matches_the_live_model_at_the_base_configuration():
    transformers = pytest.importorskip("transformers")
    torch.manual_seed(3)
    model = transformers.Wav2Vec2Model(transformers.Wav2Vec2Config()).eval()
    blob = wav2vec2.from_state_dict(BASE, model.state_dict())
    audio = cases.audio(16000, 1)
    x = torch.from_numpy(np.array(audio)).double()
    x = (x - x.mean(dim=1, keepdim=True)) / torch.sqrt(x.var(dim=1, unbiased=False, keepdim=True) + 1e-7)
    with torch.no_grad():
        want = model.double()(x)
    got = wav2vec2.reference_forward(BASE, blob, np.array(audio))
    assert cases.rel_err(got.last_hidden_state.numpy(), want.last_hidden_state.numpy()) <= TOL64
    assert cases.rel_err(got.extract_features.numpy(), want.extract_features.numpy()) <= TOL64


def test_manifest_matches_the_state_dict_of_hugging_face():
    transformers = pytest.importorskip("transformers")
    for name, c in cases.CONFIGS.items():
        hf = transformers.Wav2Vec2Config(conv_dim=list(c.conv_dim), hidden_size=c.hidden_size, num_attention_heads=c.num_attention_heads,
                                         intermediate_size=c.intermediate_size, num_hidden_layers=c.num_hidden_layers,
                                         num_conv_pos_embeddings=c.num_conv_pos_embeddings, num_conv_pos_embedding_groups=c.num_conv_pos_embedding_groups)
        state = transformers.Wav2Vec2Model(hf).state_dict()
        want = [(k, list(v.shape)) for k, v in state.items() if k != "masked_spec_embed"]
        assert [(t["name"], t["shape"]) for t in wav2vec2.manifest(c)] == want, name
        assert wav2vec2.Config.from_hf_dict(hf.to_dict()) == c, name


def test_manifest_is_dense_and_param_counts():
    assert wav2vec2.param_count(BASE) == 94371712 - 768
    for name, c in cases.CONFIGS.items():
        man, at = wav2vec2.manifest(c), 0
        for t in man:
            assert t["offset"] == at and t["count"] == int(np.prod(t["shape"]))
            at += t["count"]
        assert at == wav2vec2.param_count(c) == cases.PARAM_COUNTS[name] == cases.params(name).shape[0]
    assert wav2vec2.manifest(BASE)[0] == dict(name="feature_extractor.conv_layers.0.conv.weight", shape=[512, 1, 10], offset=0, count=5120)


def test_default_cfg_is_the_base_configuration():
    c = _lib.W2v2Cfg()
    _lib.lib().mkws_w2v2_default_cfg(ctypes.byref(c))
    want = BASE.to_c()
    assert bytes(c) == bytes(want)
    assert wav2vec2.Config.from_hf_dict({"hidden_size": 768, "vocab_size": 32, "architectures": ["Wav2Vec2ForCTC"]}) == BASE == wav2vec2.Config.base()


def test_num_frames():
    for n, T in cases.FRAMES.items():
        for c in (BASE, cases.CONFIGS["ragged"]):
            assert wav2vec2.num_frames(c, n) == T, n
    assert _lib.lib().mkws_w2v2_num_frames(ctypes.byref(BASE.to_c()), 399) <= 0
    assert _lib.lib().mkws_w2v2_num_frames(ctypes.byref(BASE.to_c()), -5) <= 0


def _named(name):
    return {k: torch.from_numpy(np.array(v)) for k, v in wav2vec2.unpack(cases.CONFIGS[name], cases.params(name)).items()}


def test_loaders_accept_both_spellings_and_the_prefix(tmp_path):
    c, blob = cases.CONFIGS["ragged"], cases.params("ragged")
    named = _named("ragged")
    assert np.array_equal(wav2vec2.from_state_dict(c, named), blob)
    old = {k.replace("parametrizations.weight.original0", "weight_g").replace("parametrizations.weight.original1", "weight_v"): v for k, v in named.items()}
    assert "encoder.pos_conv_embed.conv.weight_g" in old and np.array_equal(wav2vec2.from_state_dict(c, old), blob)
    prefixed = {"wav2vec2." + k: v for k, v in old.items()}
    prefixed.update({"wav2vec2.masked_spec_embed": torch.zeros(30), "lm_head.weight": torch.zeros(32, 30), "lm_head.bias": torch.zeros(32)})
    assert np.array_equal(wav2vec2.from_state_dict(c, prefixed), blob)
    with pytest.raises(ValueError, match="encoder.layer_norm.bias"):
        wav2vec2.from_state_dict(c, {k: v for k, v in named.items() if k != "encoder.layer_norm.bias"})
    with pytest.raises(ValueError, match="shape"):
        wav2vec2.from_state_dict(c, dict(named, **{"encoder.layer_norm.bias": torch.zeros(31)}))
    # a directory as save_pretrained leaves it, written with torch.save
    d = tmp_path / "model"
    d.mkdir()
    hf = dict(dataclass_fields(c), model_type="wav2vec2", vocab_size=32)
    (d / "config.json").write_text(json.dumps(hf))
    torch.save(prefixed, str(d / "pytorch_model.bin"))
    got_c, got = wav2vec2.from_pretrained_dir(str(d))
    assert got_c == c and np.array_equal(got, blob)
    with pytest.raises(FileNotFoundError):
        (d / "pytorch_model.bin").unlink()
        wav2vec2.from_pretrained_dir(str(d))


def dataclass_fields(c):
    import dataclasses
    return {k: (list(v) if isinstance(v, tuple) else v) for k, v in dataclasses.asdict(c).items()}


def _create(config, blob, max_batch=2, max_samples=16000):
    """-> (status, message).  A handle that came to life (a machine with a device) is destroyed."""
    L, h = _lib.lib(), ctypes.c_void_p()
    blob = np.ascontiguousarray(blob, dtype=np.float32)
    rc = L.mkws_w2v2_create(ctypes.byref(config.to_c()), blob.ctypes.data, blob.shape[0], max_batch, max_samples, ctypes.byref(h))
    msg = L.mkws_last_error().decode() if rc else ""
    if rc == 0:
        L.mkws_w2v2_destroy(h)
    return rc, msg


INVALID, UNSUPPORTED, NO_DEVICE, BAD_WEIGHTS = -1, -2, -3, -6


def test_create_refuses_before_it_looks_for_a_device():
    import dataclasses
    c, blob = cases.CONFIGS["tiny"], np.array(cases.params("tiny"))
    rep = lambda **kw: dataclasses.replace(c, **kw)
    # (the blob is the tiny one throughout: a configuration is refused before the blob is counted)
    for bad, code, word in ((rep(conv_kernel=(10, 3, 3, 3, 3, 2, 3)), UNSUPPORTED, "kernel"), (rep(conv_stride=(4, 2, 2, 2, 2, 2, 2)), UNSUPPORTED, "stride"),
                            (rep(feat_extract_norm="layer"), UNSUPPORTED, "group"), (rep(conv_bias=True), UNSUPPORTED, "conv_bias"),
                            (rep(do_stable_layer_norm=True), UNSUPPORTED, "stable"), (rep(hidden_act="gelu_new"), UNSUPPORTED, "GELU"),
                            (rep(feat_extract_activation="relu"), UNSUPPORTED, "GELU"), (rep(num_attention_heads=5), INVALID, "num_attention_heads"),
                            (rep(num_conv_pos_embedding_groups=5), INVALID, "groups"), (rep(conv_dim=(16, 16, 0, 16, 16, 16, 16)), INVALID, "conv_dim"),
                            (rep(layer_norm_eps=0.0), INVALID, "eps")):
        rc, msg = _create(bad, blob)
        assert rc == code and word in msg, (bad, rc, msg)
        with pytest.raises(ValueError):
            wav2vec2.param_count(bad)
        with pytest.raises(ValueError):
            wav2vec2.manifest(bad)
    assert _create(c, blob[:-1])[0] == BAD_WEIGHTS and "floats" in _create(c, blob[:-1])[1]
    for value in (np.nan, np.inf):
        broken = blob.copy()
        broken[777] = value
        rc, msg = _create(c, broken)
        assert rc == BAD_WEIGHTS and "777" in msg
    t = {t["name"]: t for t in wav2vec2.manifest(c)}["encoder.pos_conv_embed.conv.parametrizations.weight.original1"]
    broken = blob.copy()
    broken[t["offset"]:t["offset"] + t["count"]].reshape(t["shape"])[:, :, 3] = 0.0
    rc, msg = _create(c, broken)
    assert rc == BAD_WEIGHTS and "position 3" in msg
    for kw in (dict(max_batch=0), dict(max_samples=399)):
        assert _create(c, blob, **kw)[0] == INVALID
    assert _create(c, blob, max_batch=1 << 20, max_samples=1 << 20)[0] == UNSUPPORTED
    with pytest.raises(ValueError, match="7 layers"):
        rep(conv_dim=(7,) * 8).to_c()
    # a sound model: created where there is a device, MKWS_ERR_NO_DEVICE where there is none -- never anything else
    assert _create(c, blob)[0] in (0, NO_DEVICE)
    with pytest.raises(ValueError):
        wav2vec2.unpack(c, blob[:-1])


def test_wrapper_refuses_every_tensor_the_kernel_would_misread():
    cpu = torch.device("cpu")
    ok = torch.zeros((2, 1000), dtype=torch.float32)
    assert wav2vec2.check_audio(ok, cpu, 2, 16000) == (2, 1000)
    assert wav2vec2.check_audio(ok[:0], cpu, 2, 16000) == (0, 1000)
    for bad, word in ((ok.double(), "float32"), (ok[0], "float32 tensor"), (ok.numpy(), "ndarray"), (ok[:, ::2], "contiguous"), (ok.t().contiguous().t(), "contiguous"),
                      (torch.zeros((3, 1000)), "max_batch"), (torch.zeros((1, 399)), "samples"), (torch.zeros((1, 16001)), "samples"), (ok.to(torch.int16), "float32")):
        with pytest.raises(ValueError, match=word):
            wav2vec2.check_audio(bad, cpu, 2, 16000)
    with pytest.raises(ValueError, match="on cuda:0"):
        wav2vec2.check_audio(ok, torch.device("cuda:0"), 2, 16000)
    for bad in (torch.zeros((3, 1000)), torch.zeros((1, 399))):
        with pytest.raises(_lib.MkwsError):                              # what the library refuses too is an MkwsError as well
            wav2vec2.check_audio(bad, cpu, 2, 16000)
    with pytest.raises(ValueError, match="one flat blob"):
        wav2vec2.Wav2Vec2(cases.CONFIGS["tiny"], np.zeros((2, 13080), np.float32))
    before = dataperf_wav2vec2._model
    dataperf_wav2vec2.use_model(None)
    with pytest.raises(ValueError, match="no model"):
        dataperf_wav2vec2.get_attention(np.zeros(16000, np.float32))
    dataperf_wav2vec2.use_model(before)


def test_synthetic_weights_are_bit_stable_and_telling():
    c = cases.CONFIGS["tiny"]
    blob = wav2vec2.synthetic_weights(c, 1234)
    assert blob.dtype == np.float32 and hashlib.sha1(blob.tobytes()).hexdigest() == "263f0f7ad4ee0ba5f1c2c624d9c3605380033d10"
    assert hashlib.sha1(wav2vec2.synthetic_weights(cases.CONFIGS["ragged"], 7).tobytes()).hexdigest() == "9e4001e4ff81a9fdd80377b49269830beddb4897"
    assert not np.array_equal(blob, wav2vec2.synthetic_weights(c, 1235))
    t = wav2vec2.unpack(c, blob)
    for name, v in t.items():
        if name.endswith("layer_norm.weight"):
            assert 0.5 <= v.min() and v.max() <= 1.5 and v.std() > 0.1, name
        elif name.endswith(".bias"):
            assert 0.03 < v.std() < 0.3, name
    g = t["encoder.pos_conv_embed.conv.parametrizations.weight.original0"]
    assert g.std() > 0.01 and np.isfinite(blob).all()
    r = wav2vec2.reference_forward(c, blob, np.array(cases.audio(16000, 2)), taps=True)
    assert all(0.5 < float(s.abs().max()) < 50 for s in r.taps)


def test_few_shot_draws_are_the_references():
    keyword_files = [f"clips/bird/common_voice_{i}.wav" for i in range(260)]
    unknown_files = [f"unknown/{i}.wav" for i in range(170)]
    d = dataperf_wav2vec2.few_shot_draws(keyword_files, unknown_files)
    # the notebook's lines, on the same lists
    rng = np.random.RandomState(0)
    keyword_samples = rng.choice(keyword_files, (5 * 20) + 100, replace=False)
    unknown_samples = rng.choice(unknown_files, 20 + 100, replace=False)
    assert [keyword_files[i] for i in d["pos_test"]] == list(keyword_samples[-100:])
    assert [unknown_files[i] for i in d["negative"]] == list(unknown_samples[:20])
    assert [unknown_files[i] for i in d["neg_test"]] == list(unknown_samples[-100:])
    for ix in range(5):
        assert [keyword_files[i] for i in d["positive"][ix]] == list(keyword_samples[ix * 20:ix * 20 + 20])
    with pytest.raises(ValueError, match="draws 200 and 120"):
        dataperf_wav2vec2.few_shot_draws(keyword_files[:199], unknown_files)
    small = dataperf_wav2vec2.few_shot_draws(keyword_files[:14], unknown_files[:10], n_runs=2, n_samples=4, n_test=6, seed=3)
    assert len(small["positive"]) == 2 and len(set(np.concatenate(small["positive"] + [small["pos_test"]]))) == 14
