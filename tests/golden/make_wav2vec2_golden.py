"""Writes tests/golden/wav2vec2_golden.npz (tiny, ragged) and wav2vec2_golden_mid.npz (mid; two files keep each under 1 MiB):
Hugging Face's Wav2Vec2Model (transformers 5.15.0) in float64 at the three test configurations of tests/wav2vec2_cases.py, every
LayerNorm / GroupNorm weight, every bias and the positional kernel's g perturbed, on B = 2 clips of 400, 1000 and 16000 samples.
Run where transformers is installed:

    python tests/golden/make_wav2vec2_golden.py

Every parameter and every audio sample is rounded to a float16-representable value BEFORE the float64 run and stored as float16, which
is therefore exact and half the size.  Per configuration <name>: <name>_params (manifest order), and per length n: <name>_<n>_audio [2,n],
<name>_<n>_hidden [2,T,H], <name>_<n>_features [2,T,conv_dim[6]] (the LayerNorm'd extract_features), <name>_<n>_pooled [2,H], float64."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.join(HERE, "..", ".."), os.path.join(HERE, "..")]
from multilingual_kws_amd import wav2vec2  # noqa: E402
from wav2vec2_cases import CONFIGS, GOLDEN_FILES, GOLDEN_LENGTHS as LENGTHS  # noqa: E402


def hf_model(config, seed):
    from transformers import Wav2Vec2Config, Wav2Vec2Model
    torch.manual_seed(seed)
    hf = Wav2Vec2Config(conv_dim=list(config.conv_dim), hidden_size=config.hidden_size, num_attention_heads=config.num_attention_heads,
                        intermediate_size=config.intermediate_size, num_hidden_layers=config.num_hidden_layers,
                        num_conv_pos_embeddings=config.num_conv_pos_embeddings, num_conv_pos_embedding_groups=config.num_conv_pos_embedding_groups)
    model = Wav2Vec2Model(hf).eval()
    gen = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for name, p in model.named_parameters():
            if name.endswith("layer_norm.weight"):
                p.copy_(torch.rand(p.shape, generator=gen) + 0.5)
            elif name.endswith(".bias"):
                p.copy_(0.1 * torch.randn(p.shape, generator=gen))
            elif name.endswith("original0"):
                p.mul_(torch.rand(p.shape, generator=gen) * 0.4 + 0.8)
        for p in model.parameters():
            p.copy_(p.half().float())
    # float16 values, held in float64: the golden run sees exactly the numbers the file stores
    return model.double()


def main():
    here, files = HERE, {fname: {} for fname in GOLDEN_FILES.values()}
    for k, (name, config) in enumerate(CONFIGS.items()):
        out = files[GOLDEN_FILES[name]]
        model = hf_model(config, 100 + k)
        state = {n: v for n, v in model.state_dict().items()}
        params = wav2vec2.from_state_dict(config, state)
        assert np.array_equal(params.astype(np.float16).astype(np.float32), params)
        out[f"{name}_params"] = params.astype(np.float16)
        rng = np.random.default_rng(7 + k)
        for n in LENGTHS:
            t = np.arange(n) / 16000.0
            audio = (0.3 * np.sin(2 * np.pi * rng.uniform(100, 3000, (2, 1)) * t) + 0.1 * rng.standard_normal((2, n)) + 0.05).astype(np.float16)
            x = torch.from_numpy(audio.astype(np.float64))
            x = (x - x.mean(dim=1, keepdim=True)) / torch.sqrt(x.var(dim=1, unbiased=False, keepdim=True) + 1e-7)      # Wav2Vec2FeatureExtractor, do_normalize
            with torch.no_grad():
                r = model(x)
            hidden = r.last_hidden_state.numpy()
            out[f"{name}_{n}_audio"] = audio
            out[f"{name}_{n}_hidden"] = hidden
            out[f"{name}_{n}_features"] = r.extract_features.numpy()
            out[f"{name}_{n}_pooled"] = np.amax(hidden, axis=1)
            print(name, n, hidden.shape, "max |h|", float(np.abs(hidden).max()), "finite", bool(np.isfinite(hidden).all()))
    for fname, out in files.items():
        np.savez_compressed(os.path.join(here, fname), **out)
        print(fname, os.path.getsize(os.path.join(here, fname)), "bytes")


if __name__ == "__main__":
    main()
