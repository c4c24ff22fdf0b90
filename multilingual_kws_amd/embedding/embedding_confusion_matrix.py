"""The validation accuracy of the multilingual embedding classifier per language, and its confusion matrix (the reference's
multilingual_kws/embedding/embedding_confusion_matrix.py: the "val acc" column of the embedding table and tf.math.confusion_matrix):
every file goes through the classifier once and the per-language tallies and the matrix are taken on the device by one scorer with
groups, instead of one predict-and-compare pass per language on the host."""
import os

import numpy as np

from .. import scoring
from . import input_data


def per_language_accuracy(model, val_files, commands, language_of, model_settings=None, batch_size=1024, want_confusion=False):
    """model: an EmbeddingClassifier (predict_device gives logits over ["_silence_"] + commands).  The label of a file is
    commands.index(its parent directory) + 1 (0 is silence), its group the language code language_of(path) returns (the reference cuts
    two characters out of the path at a fixed offset; the languages are numbered in first-seen order).  Files are decoded and featurised
    on the device in batches of batch_size, as distance_filtering.embed_files(convert=True) does.
    -> ({language: accuracy}, overall accuracy), and the int64 confusion matrix [labels, labels] (row = true label) when
    want_confusion."""
    import torch
    files = [os.fspath(f) for f in val_files]
    classes = len(commands) + 1
    if classes != model.num_labels:
        raise ValueError(f"{len(commands)} commands and silence are {classes} labels, the model has {model.num_labels}")
    index = {c: i + 1 for i, c in reversed(list(enumerate(commands)))}         # list.index: the first occurrence
    words = [f.split(os.path.sep)[-2] for f in files]
    for f, w in zip(files, words):
        if w not in index:
            raise ValueError(f"{f}: its parent directory {w!r} is not in commands")
    labels = np.asarray([index[w] for w in words], dtype=np.int32)
    languages = {}
    groups = np.asarray([languages.setdefault(language_of(f), len(languages)) for f in files], dtype=np.int32)
    if not files:
        return ({}, 0.0, np.zeros((classes, classes), np.int64)) if want_confusion else ({}, 0.0)
    if model_settings is None:
        model_settings = input_data.standard_microspeech_model_settings(label_count=classes)
    dev = model.embedding.device
    scorer = scoring.Scorer(1, classes, 1, n_groups=len(languages), confusion=want_confusion, device=dev)
    d_labels, d_groups = torch.from_numpy(labels).to(dev), torch.from_numpy(groups).to(dev)

    def run():
        scorer.reset()
        with torch.cuda.device(dev):
            for s in range(0, len(files), int(batch_size)):
                e = min(s + int(batch_size), len(files))
                audio = input_data.read_clips(files[s:e], model_settings["sample_rate"], model_settings["desired_samples"], device=dev)
                spec = input_data.to_micro_spectrogram(model_settings, audio)
                scorer.add(model.predict_device(spec), d_labels[s:e], d_groups[s:e])
        return scorer.result()

    res = model.embedding.checked(run)
    by_language = {lang: float(res.group_accuracy[0, g]) for lang, g in languages.items()}
    out = (by_language, float(res.accuracy[0]))
    return out + (res.confusion_matrix[0],) if want_confusion else out
