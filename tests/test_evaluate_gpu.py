"""-m gpu: Keras' model.evaluate on the three model classes, evaluate_many, and the two consumers that came with them
(gsc_comparisons.cross_compare, embedding_confusion_matrix.per_language_accuracy), each against a by-hand evaluation of the same model
through predict: the integers with ==, the loss within the bound tests/score_cases.py derives for the scorer."""
import os
import queue

import numpy as np
import pytest

from multilingual_kws_amd import scoring
from tests import score_cases as sc
from tests.util_data import make_fewshot_dataset

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


def by_hand(probs, labels, mode):
    """score_host of one model's outputs, and the loss bound of their sum."""
    want = sc.host(dict(mode=mode, n_groups=0), probs, labels, None)
    _, sum_bound = sc.loss_bounds(dict(mode=mode, n_groups=0), probs[None], want)
    return want, float(sum_bound[0])


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    return make_fewshot_dataset(str(tmp_path_factory.mktemp("kw")), n_val=30, n_unknown=24, seed=3)


@pytest.fixture(scope="module")
def shared():
    """One frozen embedding handle and three few-shot models on it."""
    from multilingual_kws_amd.embedding import transfer_learning as tl
    from multilingual_kws_amd.head import Head, glorot_uniform_params
    emb, blob = tl.load_base_model("synthetic", max_batch=64)
    models = [tl.TransferLearnedModel(emb, Head(1024, 18, 3, max_batch=64, params=glorot_uniform_params(1024, 18, 3, 10 + k), device=emb.device), blob, "synthetic")
              for k in range(3)]
    return emb, blob, models


def eval_ds(data):
    """The reference's evaluation dataset: the keyword's files with silence and unknown mixed in, .batch(32); a fresh seeded one per pass."""
    from multilingual_kws_amd import gsc_comparisons
    return gsc_comparisons.evaluation_dataset("target", data["val"], data["unknown"], data["bg_dir"])


def test_transfer_learned_model_evaluate_on_a_clip_dataset(data, shared):
    model = shared[2][0]
    batches = [(spec.cpu().numpy(), labels.cpu().numpy()) for spec, labels in eval_ds(data)]
    specs, labels = np.concatenate([b[0] for b in batches]), np.concatenate([b[1] for b in batches])
    assert [len(b[1]) for b in batches] == [32, 16] and set(labels.tolist()) == {0, 1, 2}            # 30 keyword clips, 3 of silence, 15 unknown
    probs = np.concatenate([model.predict(b[0]) for b in batches])
    want, bound = by_hand(probs, labels, 0)
    res = model.score(eval_ds(data))
    assert res.rows.tolist() == [48] and res.correct.tolist() == [int((probs.argmax(1) == labels).sum())] and res.ignored.tolist() == [0]
    assert np.array_equal(res.confusion_matrix[0], want.confusion[0]) and res.confusion_matrix.sum() == 48
    assert abs(res.loss_sum[0] - want.loss_sum[0]) <= bound
    loss, acc = model.evaluate(eval_ds(data))
    assert acc == res.accuracy[0] == (probs.argmax(1) == labels).mean() and loss == res.loss[0] == res.loss_sum[0] / 48
    as_dict = model.evaluate(eval_ds(data), return_dict=True)
    assert as_dict == {"loss": loss, "accuracy": acc}
    # the array form, cut as the dataset was: the same calls, the same bits
    assert model.evaluate(specs, labels, batch_size=32) == [loss, acc]
    assert model.evaluate(specs[..., 0], labels.astype(np.int64), batch_size=32) == [loss, acc]
    other = model.evaluate(specs, labels, batch_size=7)
    assert other[1] == acc and abs(other[0] - loss) * 48 <= 2 * bound
    for bad in (dict(x=specs), dict(x=specs, y=labels[:-1]), dict(x=specs, y=labels.astype(np.float32)), dict(x=eval_ds(data), y=labels)):
        with pytest.raises(ValueError):
            model.evaluate(**bad)


def test_embedding_classifier_evaluate_at_761_labels():
    from multilingual_kws_amd import synth, weights
    from multilingual_kws_amd.frontend import Frontend
    from multilingual_kws_amd.train_multilingual_embedding import EmbeddingClassifier
    rng = np.random.default_rng(4)
    logits = np.concatenate([rng.uniform(-0.06, 0.06, 1024 * 761), rng.uniform(-1, 1, 761)]).astype(np.float32)
    model = EmbeddingClassifier(weights.synthetic_blob(), logits, 761, max_batch=64)
    specs = Frontend().forward(torch.from_numpy(synth.clips_float32(40)).cuda()).cpu().numpy()
    z = model.predict(specs)
    labels = np.where(np.arange(40) % 3 == 0, z.argmax(1), rng.integers(0, 761, 40)).astype(np.int64)      # a third of them right
    want, bound = by_hand(z, labels, 1)
    res = model.score(specs, labels, batch_size=32)
    assert res.rows.tolist() == [40] and res.correct.tolist() == [int(want.tally[0, 1])] and want.tally[0, 1] >= 14
    assert res.confusion_matrix.shape == (1, 761, 761) and np.array_equal(res.confusion_matrix[0], want.confusion[0])
    assert abs(res.loss_sum[0] - want.loss_sum[0]) <= bound
    ce = torch.nn.functional.cross_entropy(torch.from_numpy(z).double(), torch.from_numpy(labels)).item()
    out = model.evaluate(specs[..., None], labels, batch_size=32, return_dict=True)
    assert set(out) == {"loss", "accuracy"} and out["accuracy"] == want.tally[0, 1] / 40 and abs(out["loss"] - ce) <= 1e-12 * ce


def test_dscnn_evaluate_adds_the_l2_penalty():
    from multilingual_kws_amd import dscnn, dscnn_trainer
    params, x = dscnn.synthetic_params(7), dscnn.structured_clips(45, 11)
    rng = np.random.default_rng(6)
    model = dscnn.DSCNN(params, max_batch=16)                         # three launches for the second batch of 32
    probs = model.predict(x)
    labels = np.where(np.arange(45) % 2 == 0, probs.argmax(1), rng.integers(0, 7, 45))
    want, bound = by_hand(probs, labels, 0)
    host = dscnn.unpack(params)
    l2 = 1e-4 * sum(float(np.square(host[k].astype(np.float64)).sum()) for k in dscnn.conv_kernel_names())
    trainer = dscnn_trainer.DSCNNTrainer(params, max_batch=2)
    assert l2 > 0 and abs(model.regularization_loss() - l2) <= 1e-12 * l2 and abs(trainer.regularization_loss() - l2) <= 1e-12 * l2
    out = model.evaluate(x, labels, return_dict=True)
    assert list(out) == ["loss", "sparse_categorical_accuracy"] and out["sparse_categorical_accuracy"] == want.tally[0, 1] / 45
    assert abs((out["loss"] - model.regularization_loss()) * 45 - want.loss_sum[0]) <= bound + 45 * 4 * sc.EPS * out["loss"]
    assert model.evaluate(x, labels) == [out["loss"], out["sparse_categorical_accuracy"]]
    assert model.evaluate(x, labels, weight_decay=0.0)[0] == model.score(x, labels).loss[0]
    res = model.score(x[..., None], labels)
    assert np.array_equal(res.confusion_matrix[0], want.confusion[0])
    model.close()


def test_evaluate_many_scores_three_heads_in_one_embedding_pass(data, shared, monkeypatch):
    from multilingual_kws_amd.embedding import transfer_learning as tl
    emb, blob, models = shared
    batches = [(spec.cpu().numpy(), labels.cpu().numpy()) for spec, labels in eval_ds(data)]
    specs, own = np.concatenate([b[0] for b in batches]), np.concatenate([b[1] for b in batches])
    keyword_of_clip = np.where(own == 0, -1, np.where(own == 2, np.arange(48) % 3, 7))               # the keyword clips dealt out to three keywords
    labels = tl.keyword_labels(keyword_of_clip, 3)
    singles = [m.score(specs, labels[k], batch_size=32) for k, m in enumerate(models)]
    calls = []
    real = emb.forward
    monkeypatch.setattr(emb, "forward", lambda spec, *a, **k: (calls.append(int(spec.shape[0])), real(spec, *a, **k))[1])
    many = tl.evaluate_many(models, specs, labels=labels, batch_size=32)
    assert calls == [32, 16]                                          # one embedding forward per batch, whatever the number of heads
    for k in range(3):
        assert many[k]["rows"] == 48 and np.array_equal(many[k]["confusion_matrix"], singles[k].confusion_matrix[0])
        assert many[k]["accuracy"] == singles[k].accuracy[0] and many[k]["loss"] == singles[k].loss[0]       # forward_many has Head.forward's bits
        pr, rc, f1 = scoring.precision_recall_f1(many[k]["confusion_matrix"])
        assert f1.shape == (3,) and np.all((0 <= f1) & (f1 <= 1))
    assert len({m["confusion_matrix"].tobytes() for m in many}) == 3
    # shared labels, and a dataset with its own labels
    calls.clear()
    shared_labels = tl.evaluate_many(models, specs, own, batch_size=1024, return_dict=False)
    assert calls == [48] and [r[1] for r in shared_labels] == [m.score(specs, own).accuracy[0] for m in models]
    from_ds = tl.evaluate_many(models[:2], eval_ds(data))
    assert [r["accuracy"] for r in from_ds] == [r[1] for r in shared_labels[:2]]
    # a model on another handle is scored in its own pass and handed back in its place
    emb2, _ = tl.load_base_model("synthetic", max_batch=64)            # the same weights behind a second handle
    stranger = tl.TransferLearnedModel(emb2, models[1].head, None, "synthetic")
    mixed = tl.evaluate_many([models[0], stranger, models[2]], specs, labels=labels, batch_size=32)
    assert mixed[0]["loss"] == many[0]["loss"] and mixed[2]["loss"] == many[2]["loss"]
    assert np.array_equal(mixed[1]["confusion_matrix"], stranger.score(specs, labels[1]).confusion_matrix[0]) and mixed[1]["loss"] == many[1]["loss"]
    with pytest.raises(ValueError):
        tl.evaluate_many(models, specs, labels=labels[:2])
    with pytest.raises(ValueError):
        tl.evaluate_many(models, specs)


def test_per_language_accuracy_on_two_made_up_languages(tmp_path):
    from multilingual_kws_amd import synth, weights
    from multilingual_kws_amd.embedding import input_data
    from multilingual_kws_amd.embedding.embedding_confusion_matrix import per_language_accuracy
    from multilingual_kws_amd.train_multilingual_embedding import EmbeddingClassifier
    commands = ["uno", "dos", "tres", "vier"]
    rng = np.random.default_rng(8)
    logits = np.concatenate([rng.uniform(-0.3, 0.3, 1024 * 5), [-1e4, 0, 0, 0, 0]]).astype(np.float32)       # (a bias that rules silence out)
    model = EmbeddingClassifier(weights.synthetic_blob(), logits, 5, commands=commands, max_batch=64)
    audio = torch.from_numpy(synth.clips_float32(14)).cuda()
    first = model.predict(input_data.to_micro_spectrogram(input_data.standard_microspeech_model_settings(5), audio).cpu().numpy()).argmax(1)
    words = [commands[(int(p) - 1) % 4] if i % 2 == 0 else commands[i % 4] for i, p in enumerate(first)]   # every other file under the word the model says
    paths = [str(tmp_path / ("xx" if i < 9 else "yy") / "clips" / w / f"c{i}.wav") for i, w in enumerate(words)]
    input_data.write_clips(audio, paths)
    language_of = lambda p: p.split(os.path.sep)[-4]
    by_language, overall, cm = per_language_accuracy(model, paths, commands, language_of, batch_size=8, want_confusion=True)
    # by hand: one predict over the files as written
    settings = input_data.standard_microspeech_model_settings(5)
    pred = model.predict(input_data.to_micro_spectrogram(settings, input_data.read_clips(paths, 16000, 16000)).cpu().numpy()).argmax(1)
    truth = np.asarray([commands.index(w) + 1 for w in words])
    lang = np.asarray([language_of(p) for p in paths])
    assert list(by_language) == ["xx", "yy"] and by_language == {l: float((pred == truth)[lang == l].mean()) for l in ("xx", "yy")}
    assert overall == float((pred == truth).mean()) and 0 < overall < 1
    want = np.zeros((5, 5), np.int64)
    np.add.at(want, (truth, pred), 1)
    assert cm.dtype == np.int64 and np.array_equal(cm, want)
    assert per_language_accuracy(model, paths, commands, language_of) == (by_language, overall)
    assert per_language_accuracy(model, [], commands, language_of) == ({}, 0.0)
    with pytest.raises(ValueError):
        per_language_accuracy(model, paths, commands[:3], language_of)


def test_cross_compare_end_to_end_on_a_tiny_file_tree(data, tmp_path):
    from multilingual_kws_amd import gsc_comparisons as gsc
    other = make_fewshot_dataset(str(tmp_path / "other_corpus"), n_train=0, n_val=12, n_unknown=10, seed=9)
    c = gsc.CrossCompare(keyword="target", train_files=data["train"], val_files=data["val"][:8], test_files=data["val"][8:], cross_testset=other["val"],
                         unknown_test=data["unknown"][12:], unknown_cross=other["unknown"])
    q = queue.Queue()
    test_acc, cross_acc, model = gsc.cross_compare(c, q, base_model_path="synthetic", unknown_files=data["unknown"][:12], bg_datadir=data["bg_dir"], seed=2,
                                                   return_model=True)
    assert q.get_nowait() == (test_acc, cross_acc) and 0.0 <= test_acc <= 1.0 and 0.0 <= cross_acc <= 1.0
    assert model.history is not None and len(model.history["val_accuracy"]) == 4                      # the reference's four epochs
    for files, unknown, got in ((c.test_files, c.unknown_test, test_acc), (c.cross_testset, c.unknown_cross, cross_acc)):
        right = seen = 0
        for spec, labels in gsc.evaluation_dataset("target", files, unknown, data["bg_dir"]):
            right += int((model.predict(spec.cpu().numpy()).argmax(1) == labels.cpu().numpy()).sum())
            seen += len(labels)
        assert seen == len(files) + int(len(files) * 0.1) + int(len(files) * 0.5) and got == right / seen
    assert gsc.load_gsc_data("target", os.path.dirname(os.path.dirname(data["val"][0])))[3] == sorted(data["unknown"])
