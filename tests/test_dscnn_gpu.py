"""The DS-CNN on the device (mkws_dscnn_*, multilingual_kws_amd/dscnn.py, dscnn_comparison.py) against its float64 specification
dscnn_host, which tests/test_dscnn_cpu.py holds to an independent restatement; that file also asserts what makes the inputs telling.

Bounds: every tensor (stages 0..5, logits) within 1e-5 * max |reference|, the bound tests/test_embedding_gpu.py uses for such
comparisons; probabilities within 1e-5 * max(1, max |logit|), since a softmax moves by at most half the largest logit error; the argmax
equal on every row whose reference top-2 gap is at least 1e-4 * max |logit| (test_dscnn_cpu.py caps the rows below it at 5 %)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import dscnn_cases as cases  # noqa: E402

from multilingual_kws_amd import _lib, dscnn, dscnn_comparison, synth  # noqa: E402
from multilingual_kws_amd.embedding import input_data, transfer_learning  # noqa: E402

pytestmark = pytest.mark.gpu
TOL = 1e-5


@pytest.fixture(scope="module")
def models():
    made = {L: dscnn.DSCNN(cases.params(L), L, max_batch=1024) for L in cases.LABEL_COUNTS}
    yield made
    for m in made.values():
        m.close()


def _cuda(a):
    return torch.from_numpy(np.array(a)).cuda()             # (a copy: the shared cases are read-only)


def _close(got, want, what):
    err = float(np.abs(got.astype(np.float64) - want).max())
    assert got.shape == want.shape and err <= TOL * np.abs(want).max(), (what, err / np.abs(want).max())


def _check_heads(m, x, want_logits, what):
    logits, probs = m.logits(x).cpu().numpy(), m.forward(x).cpu().numpy()
    _close(logits, want_logits, (what, "logits"))
    scale = np.abs(want_logits).max()
    assert np.abs(probs.astype(np.float64) - dscnn.softmax_host(want_logits)).max() <= TOL * max(1.0, scale), what
    top2 = np.sort(want_logits, axis=1)[:, -2:]
    clear = (top2[:, 1] - top2[:, 0]) >= 1e-4 * scale
    assert np.array_equal(probs.argmax(axis=1)[clear], want_logits.argmax(axis=1)[clear]), what
    assert np.array_equal(logits.argmax(axis=1)[clear], want_logits.argmax(axis=1)[clear]), what


@pytest.mark.parametrize("B", cases.BATCHES + ("grid+3",))
@pytest.mark.parametrize("label_count", cases.LABEL_COUNTS)
def test_every_stage_matches_the_specification(models, label_count, B):
    m = models[label_count]
    big = B == "grid+3"
    if big:                                            # more clips than workgroups: the per-workgroup clip loop (mkws_dscnn_grid)
        B = m.grid + 3
        assert 0 < m.grid and B <= m.max_batch
    n = B if big else max(cases.BATCHES)
    x = _cuda(cases.clips(n)[:B])
    stages = cases.trunk_reference(n)
    for stage in range(6):
        _close(m.tap(x, stage).cpu().numpy(), stages[stage][:B], (label_count, B, stage))
    _check_heads(m, x, cases.logits_reference(n, label_count)[:B], (label_count, B))


def test_deterministic_clips(models):
    det, names = cases.deterministic_clips()
    m = models[7]
    stages, logits = dscnn.dscnn_host(det, cases.params(7), "all")
    x = torch.from_numpy(det).cuda()
    for stage in range(6):
        got = m.tap(x, stage).cpu().numpy()
        for i, name in enumerate(names):                 # clip by clip: full scale must not set the bound for an impulse
            _close(got[i], stages[stage][i], (name, stage))
    for i, name in enumerate(names):
        _check_heads(m, x[i:i + 1], logits[i:i + 1], name)


def test_row24_feeds_row23_and_is_not_pooled():
    x, a, b = cases.row24_pair()
    d_x = torch.from_numpy(x).cuda()
    got = []
    for p in (a, b):
        m = dscnn.DSCNN(p, max_batch=4)
        stages, logits = dscnn.dscnn_host(x, p, "all")
        for stage in range(6):
            _close(m.tap(d_x, stage).cpu().numpy(), stages[stage], stage)
        _close(m.logits(d_x).cpu().numpy(), logits, "logits")
        s4, s5 = m.tap(d_x, 4).cpu().numpy().astype(np.float64), m.tap(d_x, 5).cpu().numpy()
        assert np.abs(s4[:, 24]).max() > 0
        _close(s5, s4[:, :24].mean(axis=(1, 2)), "pool of the device's own rows 0..23")
        got.append((m.tap(d_x, 0).cpu().numpy(), m.logits(d_x).cpu().numpy()))
        m.close()
    assert np.array_equal(got[0][0][:, :24], got[1][0][:, :24]) and not np.array_equal(got[0][0][:, 24], got[1][0][:, 24])
    assert np.abs(got[0][1] - got[1][1]).max() > 1e-3 * np.abs(got[0][1]).max()


def test_empty_batch_and_batch_above_max_batch():
    m = dscnn.DSCNN(cases.params(7), max_batch=4)
    assert m.forward(torch.zeros((0, 49, 40), device="cuda")).shape == (0, 7)
    assert m.tap(torch.zeros((0, 49, 40), device="cuda"), 2).shape == (0, 25, 20, 64)
    x = _cuda(cases.clips(5))
    with pytest.raises(_lib.MkwsError) as e:
        m.forward(x)
    assert e.value.code == -1
    with pytest.raises(_lib.MkwsError):
        m.tap(x, 0)
    with pytest.raises(_lib.MkwsError):
        m.tap(x[:2], 6)
    # predict batches by max_batch instead
    want = dscnn.softmax_host(cases.logits_reference(max(cases.BATCHES), 7)[:5])
    for arr in (cases.clips(5), cases.clips(5)[..., None]):
        got = m.predict(arr)
        assert isinstance(got, np.ndarray) and got.shape == (5, 7) and np.abs(got - want).max() <= TOL
    m.close()


def test_two_forwards_are_bit_identical_and_streams_are_honoured(models):
    m = models[12]
    x = _cuda(cases.clips(67))
    first, second = m.forward(x), m.forward(x)
    assert torch.equal(first, second) and torch.equal(m.logits(x), m.logits(x))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        third = m.forward(x)
        fourth = m.tap(x, 4)
    side.synchronize()
    assert torch.equal(first, third) and torch.equal(fourth, m.tap(x, 4))


@pytest.fixture(scope="module")
def wav_files(tmp_path_factory):
    root = tmp_path_factory.mktemp("dscnn_wavs")
    pcm = synth.clips_int16(6, seed=0xD5C0)
    files = []
    for i in range(6):
        path = root / f"clip{i}.wav"
        path.write_bytes(synth.wav_bytes(pcm[i]))
        files.append(str(path))
    return files


def test_evaluate_counts_accuracy_and_confusion_on_files(models, wav_files):
    ms = input_data.standard_microspeech_model_settings(3)
    m = models[7]
    specs = transfer_learning._specs_for_files(wav_files, ms)
    ref = dscnn.dscnn_host(specs, cases.params(7))
    top2 = np.sort(ref, axis=1)[:, -2:]
    assert ((top2[:, 1] - top2[:, 0]) >= 1e-4 * np.abs(ref).max()).all(), "a file's reference classes are too close to call: change the seed"
    want = ref.argmax(axis=1)
    labels = np.asarray([int(want[0]), int(want[1]), (int(want[2]) + 1) % 7, int(want[3]), (int(want[4]) + 3) % 7, int(want[5])])
    confusion = np.zeros((7, 7), np.int64)
    for t, p in zip(labels, want):
        confusion[t, p] += 1
    for convert in (False, True):
        got = dscnn_comparison.evaluate(m, wav_files, labels, ms, convert=convert)
        assert got["predictions"].tolist() == want.tolist(), convert
        assert got["accuracy"] == 4 / 6 and got["confusion_matrix"].dtype == np.int64 and np.array_equal(got["confusion_matrix"], confusion)
    with pytest.raises(ValueError):
        dscnn_comparison.evaluate(m, wav_files, labels[:5], ms)
    # the model goes unchanged into the few-shot evaluation helpers
    split = transfer_learning.evaluate_files_multiclass(wav_files, int(want[0]), m, ms)
    probs = m.predict(specs)
    assert len(split["correct"]) == int((want == want[0]).sum()) and len(split["correct"]) + len(split["incorrect"]) == 6
    assert sorted(split["correct"] + split["incorrect"]) == sorted(probs.max(axis=1).tolist())


def test_model_def_builds_the_untrained_network():
    m = dscnn_comparison.model_def(12, seed=3, max_batch=8)
    assert m.label_count == 12 and m.params.shape == (24908,)
    t = dscnn.unpack(m.params)
    assert not t["conv2d/bias"].any() and not t["dense/bias"].any() and (t["batch_normalization_4/gamma"] == 1).all()
    assert np.abs(t["conv2d/kernel"]).max() <= np.sqrt(6.0 / (40 + 40 * 64)) and np.abs(t["dense/kernel"]).max() <= np.sqrt(6.0 / (64 + 12))
    x = cases.clips(8)
    want = dscnn.dscnn_host(x, m.params)
    _close(m.logits(_cuda(x)).cpu().numpy(), want, "model_def logits")
    probs = m.predict(x)
    assert np.allclose(probs.sum(axis=1), 1.0, atol=1e-5)
    m.close()
