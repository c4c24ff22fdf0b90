"""The wav2vec 2.0 encoder on the device (mkws_w2v2_*, multilingual_kws_amd/wav2vec2.py, dataperf_wav2vec2.py) against its float64
specification wav2vec2.reference_forward, which tests/test_wav2vec2_cpu.py holds to Hugging Face's own float64 forward.

Bound.  The yardstick is the float32 evaluation of the specification on the CPU: E32 = max |reference(float32) - reference(float64)| /
max |float64|, computed here for every case.  The device must lie within FACTOR = 4 times the largest E32 over a test's cases, relative
to max |float64| of the tensor compared; the factor covers what legitimately differs from torch's float32: the K-blocked summation
order of the MFMA GEMM and the device's own erf / exp.  Measured on an MI355X: the device between 1.6e-7 and 1.1e-6 over every case
of this file (E32 between 1.4e-7 and 1.9e-6), 8.4e-7 at the base configuration (E32 6.5e-7); the tables are in DESIGN.md section 39 and
profiles/wav2vec2_bench.txt.  Every test prints its figures before it asserts (run with -s)."""
import ctypes
import os
import sys
import wave

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import wav2vec2_cases as cases  # noqa: E402

from multilingual_kws_amd import _lib, dataperf_wav2vec2, logreg, wav2vec2  # noqa: E402

pytestmark = pytest.mark.gpu
NAMES = sorted(cases.CONFIGS)


@pytest.fixture(scope="module")
def models():
    made = {name: wav2vec2.Wav2Vec2(cases.CONFIGS[name], cases.params(name), max_batch=cases.MAX_BATCH, max_samples=16000) for name in NAMES}
    yield made
    for m in made.values():
        m.close()


def _cuda(a):
    return torch.from_numpy(np.array(a)).cuda()             # (a copy: the shared cases are read-only)


def _bound(e32s):
    return cases.FACTOR * max(e32s)


def _check(got, want, bound, what):
    err = cases.rel_err(got.cpu().numpy(), want)
    print(f"{what}: device error {err:.3e}, bound {bound:.3e}")
    assert err <= bound, (what, err, bound)


def test_forward_and_embed_match_the_specification(models):
    grid = [(name, n, B) for name in NAMES for n in cases.LENGTHS for B in cases.BATCHES]
    bound = _bound([cases.case(*k).e32 for k in grid] + [cases.case(*k).e32_embed for k in grid])
    for name, n, B in grid:
        c, m = cases.case(name, n, B), models[name]
        hidden, embed = m.forward_embed(_cuda(c.audio))
        assert tuple(hidden.shape) == (B, cases.FRAMES[n], m.hidden_size) and tuple(embed.shape) == (B, m.hidden_size)
        _check(hidden, c.hidden, bound, (name, n, B, "hidden", f"E32 {c.e32:.3e}"))
        _check(embed, c.embed, bound, (name, n, B, "embed", f"E32 {c.e32_embed:.3e}"))
        assert torch.equal(embed, hidden.amax(dim=1))


def test_forward_and_embed_match_the_golden_files(models):
    grid = [(name, n) for name in NAMES for n in cases.GOLDEN_LENGTHS]
    bound = _bound([cases.golden_case(*k).e32 for k in grid] + [cases.golden_case(*k).e32_embed for k in grid])
    for name, n in grid:
        g, m = cases.golden(name), models[name]
        hidden, embed = m.forward_embed(_cuda(g[f"{n}_audio"]))
        _check(hidden, g[f"{n}_hidden"], bound, (name, n, "golden hidden"))
        _check(embed, g[f"{n}_pooled"], bound, (name, n, "golden pooled"))


@pytest.mark.parametrize("name", ("tiny", "ragged"))
def test_every_tap_stage_matches_the_specification(models, name):
    m = models[name]
    grid = [(name, n, B) for n in (400, 721, 4000, 16000) for B in (1, 3)]
    stages = 10 + cases.CONFIGS[name].num_hidden_layers
    bound = _bound([e for k in grid for e in cases.case(*k).e32_taps])
    for k in grid:
        c = cases.case(*k)
        assert len(c.taps) == stages
        x = _cuda(c.audio)
        for stage in range(stages):
            got = m.tap(x, stage)
            assert tuple(got.shape) == c.taps[stage].shape
            _check(got, c.taps[stage], bound, (k, "stage", stage, f"E32 {c.e32_taps[stage]:.3e}"))
    with pytest.raises(ValueError, match="stage"):
        m.tap(x, stages)


def test_normalize_off_takes_the_audio_as_given(models):
    m = models["mid"]
    on, off = cases.case("mid", 4000, 3), cases.case("mid", 4000, 3, False)
    bound = _bound([on.e32, off.e32])
    x = _cuda(on.audio)
    try:
        m.normalize = False
        _check(m.forward(x), off.hidden, bound, "normalize off")
        assert torch.equal(m.tap(x, 0), x)
    finally:
        m.normalize = True
    _check(m.forward(x), on.hidden, bound, "normalize on")
    # The GroupNorm behind layer 0 removes most of what the processor does (a constant offset and a scale): the two specifications differ by
    # what the epsilons leave, 2.6e-4 here -- still far outside the bound, so a device that ignored the switch would fail above.
    assert cases.rel_err(off.hidden, on.hidden) > 10 * bound and cases.rel_err(off.taps[0], on.taps[0]) > 0.5


def test_outputs_alone_twice_and_inside_canaries(models):
    """d_hidden alone, d_embed alone and both give the same bits, twice over, and nothing is written outside exactly [B,T,H] and [B,H]."""
    L = _lib.lib()
    for name in NAMES:
        m, (n, B) = models[name], (4000, 3)
        T, H = cases.FRAMES[n], m.hidden_size
        x = _cuda(cases.audio(n, B))
        both_h, both_e = m.forward_embed(x)
        assert torch.equal(m.forward(x), both_h) and torch.equal(m.embed(x), both_e)
        assert torch.equal(m.forward_embed(x)[0], both_h) and torch.equal(m.forward_embed(x)[1], both_e)
        pad, canary = 61, -777.25
        for want_h, want_e in ((True, False), (False, True), (True, True)):
            buf_h = torch.full((pad + B * T * H + pad,), canary, dtype=torch.float32, device="cuda")
            buf_e = torch.full((pad + B * H + pad,), canary, dtype=torch.float32, device="cuda")
            _lib.check(L.mkws_w2v2_forward(m.h, ctypes.c_void_p(x.data_ptr()), B, n, 1, ctypes.c_void_p(buf_h.data_ptr() + 4 * pad) if want_h else None,
                                           ctypes.c_void_p(buf_e.data_ptr() + 4 * pad) if want_e else None, _lib.current_stream_ptr()))
            for buf, want, ref in ((buf_h, want_h, both_h), (buf_e, want_e, both_e)):
                inner = buf[pad:buf.numel() - pad]
                assert bool((buf[:pad] == canary).all()) and bool((buf[buf.numel() - pad:] == canary).all()), (name, "canary")
                assert torch.equal(inner, ref.reshape(-1)) if want else bool((inner == canary).all()), (name, want_h, want_e)
    # the library's own refusals, all host-side
    m = models["tiny"]
    x = _cuda(cases.audio(4000, 3))
    ptr, out = ctypes.c_void_p(x.data_ptr()), ctypes.c_void_p(both_h.data_ptr())
    assert L.mkws_w2v2_forward(m.h, ptr, 3, 4000, 1, None, None, None) == -1
    assert L.mkws_w2v2_forward(m.h, ptr, 4, 3000, 1, out, None, None) == -1 and b"max_batch" in L.mkws_last_error()
    assert L.mkws_w2v2_forward(m.h, ptr, 1, 16001, 1, out, None, None) == -1
    assert L.mkws_w2v2_forward(m.h, ptr, 1, 399, 1, out, None, None) == -1
    assert L.mkws_w2v2_forward(m.h, ptr, 0, 4000, 1, None, None, None) == 0
    assert L.mkws_w2v2_tap(m.h, ptr, 1, 4000, 1, 12, out, None) == -1
    assert tuple(m.forward(x[:0]).shape) == (0, 12, 32) and tuple(m.embed(x[:0]).shape) == (0, 32)
    with pytest.raises(ValueError, match="contiguous"):
        m.forward(x[:, ::2])
    with pytest.raises(_lib.MkwsValueError):
        m.forward(torch.cat([x, x]))
    with pytest.raises(ValueError, match="float32 tensor"):
        m.embed(x.cpu())


def test_captured_forward_replays_the_eager_bits(models):
    m = models["mid"]
    first, second = _cuda(cases.audio(16000, 3)), _cuda(cases.audio(16000, 3, seed=1))
    eager_first, eager_second = m.forward_embed(first), m.forward_embed(second)
    assert not torch.equal(eager_first[0], eager_second[0])
    static = first.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        m.forward_embed(static)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        hidden, embed = m.forward_embed(static)
    for audio, want in ((second, eager_second), (first, eager_first)):
        static.copy_(audio)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(hidden, want[0]) and torch.equal(embed, want[1])


def test_base_configuration_on_synthetic_weights():
    config = wav2vec2.Config.base()
    blob = wav2vec2.synthetic_weights(config, 1234)
    c = cases.Case(config, blob, cases.audio(16000, 2))
    with wav2vec2.Wav2Vec2(config, blob, max_batch=2) as m:
        hidden, embed = m.forward_embed(_cuda(c.audio))
        _check(hidden, c.hidden, _bound([c.e32]), ("base", "hidden", f"E32 {c.e32:.3e}"))
        _check(embed, c.embed, _bound([c.e32_embed]), ("base", "embed", f"E32 {c.e32_embed:.3e}"))


def test_split_reductions_on_the_guarded_gemm_route():
    """Widths that are no multiple of 4 (the GEMM's guarded kernel) with reductions long enough to be split into slices (66 and 70
    columns: two slices each), which none of the three shared configurations combines."""
    config = wav2vec2.Config(conv_dim=(6, 22, 22, 10, 10, 10, 14), hidden_size=30, num_attention_heads=3, intermediate_size=70, num_hidden_layers=2,
                             num_conv_pos_embeddings=5, num_conv_pos_embedding_groups=5)
    blob = wav2vec2.synthetic_weights(config, 5)
    c = cases.Case(config, blob, cases.audio(4000, 3))
    with wav2vec2.Wav2Vec2(config, blob, max_batch=3) as m:
        x = _cuda(c.audio)
        bound = _bound(c.e32_taps)
        for stage in (3, 4, 8, 10, 11):
            _check(m.tap(x, stage), c.taps[stage], bound, ("guarded split", "stage", stage, f"E32 {c.e32_taps[stage]:.3e}"))
        hidden, embed = m.forward_embed(x)
        _check(hidden, c.hidden, _bound([c.e32]), ("guarded split", "hidden", f"E32 {c.e32:.3e}"))
        _check(embed, c.embed, _bound([c.e32_embed]), ("guarded split", "embed", f"E32 {c.e32_embed:.3e}"))


def _write_wav(path, samples):
    with wave.open(str(path), "wb") as f:
        f.setnchannels(1)
        f.setsampwidth(2)
        f.setframerate(16000)
        f.writeframes(np.asarray(samples, dtype="<i2").tobytes())


def _keyword_files(tmp_path, kind, count, freq, seed):
    """One-second 16-bit clips of a 'keyword': a tone of the keyword's frequency with a clip-dependent onset and level, over noise."""
    rng = np.random.default_rng(seed)
    t = np.arange(16000) / 16000.0
    files, pcm = [], []
    for i in range(count):
        x = rng.uniform(0.2, 0.5) * np.sin(2 * np.pi * freq * rng.uniform(0.97, 1.03) * t) * (t > rng.uniform(0.0, 0.4)) + 0.03 * rng.standard_normal(16000)
        samples = np.round(x * 32767).clip(-32768, 32767).astype(np.int16)
        files.append(tmp_path / f"{kind}_{i}.wav")
        pcm.append(samples)
        _write_wav(files[-1], samples)
    return files, np.stack(pcm)


def test_embed_files_reads_wav_files(models, tmp_path):
    m = models["tiny"]
    files, pcm = _keyword_files(tmp_path, "clip", 5, 440.0, 1)
    audio = (pcm.astype(np.float32) / np.float32(32768.0))
    c = cases.Case(cases.CONFIGS["tiny"], cases.params("tiny"), audio)
    got = dataperf_wav2vec2.embed_files(files, batch=2, model=m)              # batches of 2, 2, 1
    _check(got, c.embed, _bound([c.e32_embed]), "embed_files")
    dataperf_wav2vec2.use_model(m)
    try:
        one = dataperf_wav2vec2.get_embedding_from_fp(files[3])
        assert one.shape == (32,) and np.array_equal(one, got[3].cpu().numpy())
        hidden = dataperf_wav2vec2.get_attention(audio[3])
        assert tuple(hidden.shape) == (1, 49, 32) and np.array_equal(hidden[0].amax(dim=0).cpu().numpy(), one)
    finally:
        dataperf_wav2vec2.use_model(None)


def test_few_shot_runs_agree_with_the_host_route(models, tmp_path):
    m = models["mid"]
    n_runs, n_samples, n_test = 2, 4, 6
    keyword_files, _ = _keyword_files(tmp_path, "keyword", n_runs * n_samples + n_test + 3, 350.0, 2)
    unknown_files, _ = _keyword_files(tmp_path, "unknown", n_samples + n_test + 2, 1900.0, 3)
    acc, d = dataperf_wav2vec2.few_shot_runs(keyword_files, unknown_files, n_runs=n_runs, n_samples=n_samples, n_test=n_test, seed=0, batch=3, model=m,
                                             details=True)
    assert len(acc) == n_runs and d["bank"].shape == (n_samples + 2 * n_test + n_runs * n_samples, 96)
    bank = d["bank"].cpu().numpy()
    for r in range(n_runs):
        rows = d["rows"][d["offsets"][r]:d["offsets"][r + 1]]
        host = logreg.logreg_host(bank, rows, d["labels"][d["offsets"][r]:d["offsets"][r + 1]], 2, C=1.0)
        pred, probs = logreg.predict_host(bank, d["test_rows"], host.coef, host.intercept)
        clear = np.abs(probs[:, 1] - 0.5) > 1e-3                              # (a row on the boundary may fall either way)
        assert clear.sum() >= n_test
        assert np.array_equal(d["pred"][r][clear], pred[clear]), r
        assert acc[r] == float((d["pred"][r] == d["test_labels"]).mean())
    assert dataperf_wav2vec2.few_shot_runs(keyword_files, unknown_files, n_runs=n_runs, n_samples=n_samples, n_test=n_test, seed=0, batch=3, model=m) == acc
