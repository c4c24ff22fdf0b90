"""The reference's wav2vec 2.0 baseline (notebooks/dataperf_wav2vec2.py) on the device: get_attention and get_embedding_from_fp are
the notebook's functions over wav2vec2.Wav2Vec2 (one clip: the last hidden state, and its maximum over time), embed_files embeds many
files in batches, few_shot_runs is the notebook's experiment (:93-132): N_RUNS logistic regressions on 20 + 20 embeddings, scored on
100 + 100, the draws through np.random.RandomState(seed).choice in the notebook's order, the fit and the score through logreg's device
path (LogisticRegression() defaults = C 1, no scaler).  The model is whatever use_model() was given last: weights are loaded from
local files (wav2vec2.from_pretrained_dir), nothing is fetched."""
import numpy as np

from . import logreg, wav2vec2
from .embedding import input_data

SAMPLE_RATE = 16000
_model = None


def use_model(model):
    """The wav2vec2.Wav2Vec2 the functions below run (the notebook's module-level `model`).  -> the model."""
    global _model
    _model = model
    return model


def _current(model):
    model = model if model is not None else _model
    if model is None:
        raise ValueError("no model: call dataperf_wav2vec2.use_model(wav2vec2.Wav2Vec2(...)) first, or pass model=")
    return model


def get_attention(audio, model=None):
    """One clip of 16 kHz samples (numpy [n] or a float32 CUDA tensor [n]) -> its last hidden state, CUDA [1, T, H]."""
    import torch
    model = _current(model)
    if not torch.is_tensor(audio):
        audio = torch.from_numpy(np.array(audio, dtype=np.float32))
    audio = audio.to(model.device, dtype=torch.float32).reshape(1, -1).contiguous()
    return model.forward(audio)


def embed_files(files, batch=32, model=None):
    """WAV files of any supported format, rate and channel count -> CUDA [len(files), H]: every file brought to 16 kHz mono and one second
    on the device (input_data.read_clips), then one embed per batch of at most min(batch, model.max_batch) clips."""
    import torch
    model = _current(model)
    files = list(files)
    step = max(1, min(int(batch), model.max_batch))
    n = min(SAMPLE_RATE, model.max_samples)
    outs = [model.embed(input_data.read_clips(files[s:s + step], sample_rate=SAMPLE_RATE, desired_samples=n, device=model.device).contiguous())
            for s in range(0, len(files), step)]
    return torch.cat(outs) if outs else torch.empty((0, model.hidden_size), dtype=torch.float32, device=model.device)


def get_embedding_from_fp(filepath, model=None):
    """One file -> its embedding, numpy [H] (the notebook's np.amax(last_hidden_state, axis=0))."""
    return embed_files([filepath], batch=1, model=model)[0].cpu().numpy()


def few_shot_draws(keyword_files, unknown_files, n_runs=5, n_samples=20, n_test=100, seed=0):
    """The notebook's draws (:101-107, :119-122) as indices into the two lists: dict(positive = [n_runs][n_samples] keyword indices,
    negative = [n_samples] unknown indices, pos_test = [n_test] keyword indices, neg_test = [n_test] unknown indices).  The same
    RandomState draws the keywords first, then the unknowns, both without replacement."""
    n_kw, n_unk = int(n_runs) * int(n_samples) + int(n_test), int(n_samples) + int(n_test)
    if len(keyword_files) < n_kw or len(unknown_files) < n_unk:
        raise ValueError(f"{len(keyword_files)} keyword and {len(unknown_files)} unknown files, the experiment draws {n_kw} and {n_unk}")
    rng = np.random.RandomState(seed)
    kw = rng.choice(len(keyword_files), n_kw, replace=False)
    unk = rng.choice(len(unknown_files), n_unk, replace=False)
    return dict(positive=[kw[i * n_samples:(i + 1) * n_samples] for i in range(n_runs)], negative=unk[:n_samples], pos_test=kw[n_kw - n_test:],
                neg_test=unk[n_unk - n_test:])


def few_shot_runs(keyword_files, unknown_files, n_runs=5, n_samples=20, n_test=100, seed=0, batch=32, model=None, details=False):
    """The notebook's experiment -> the test accuracy of every run, [n_runs] floats.  Every drawn file is embedded once into one bank;
    the n_runs problems (positives of the run + the shared negatives, labels 1 / 0) are fitted in one logreg.fit_on_device call and
    scored in one logreg.score_on_device call on pos_test + neg_test.  details=True -> (accuracies, dict(bank = CUDA [rows, H], rows,
    labels, offsets, test_rows, test_labels, pred = int32 [n_runs, 2 * n_test], fit = the LogregFit))."""
    d = few_shot_draws(keyword_files, unknown_files, n_runs, n_samples, n_test, seed)
    order = [("u", int(i)) for i in d["negative"]] + [("k", int(i)) for i in d["pos_test"]] + [("u", int(i)) for i in d["neg_test"]]
    order += [("k", int(i)) for run in d["positive"] for i in run]
    bank = embed_files([keyword_files[i] if kind == "k" else unknown_files[i] for kind, i in order], batch=batch, model=model)
    neg = np.arange(n_samples)
    test_rows = np.arange(n_samples, n_samples + 2 * n_test)
    test_labels = np.concatenate([np.ones(n_test, np.int32), np.zeros(n_test, np.int32)])
    first = n_samples + 2 * n_test
    rows = np.concatenate([np.concatenate([first + r * n_samples + np.arange(n_samples), neg]) for r in range(n_runs)]).astype(np.int32)
    labels = np.tile(np.concatenate([np.ones(n_samples, np.int32), np.zeros(n_samples, np.int32)]), n_runs)
    offsets = np.arange(n_runs + 1, dtype=np.int32) * (2 * n_samples)
    fit = logreg.fit_on_device(bank, rows, labels, offsets, 2, C=1.0, standardize=False)
    pred, correct, _, _ = logreg.score_on_device(bank, np.tile(test_rows, n_runs).astype(np.int32), np.tile(test_labels, n_runs),
                                                 np.arange(n_runs + 1, dtype=np.int32) * (2 * n_test), fit.d_coef, fit.d_intercept)
    acc = [float(c) / (2 * n_test) for c in correct.cpu().numpy()]
    if not details:
        return acc
    return acc, dict(bank=bank, rows=rows, labels=labels, offsets=offsets, test_rows=test_rows, test_labels=test_labels,
                     pred=pred.cpu().numpy().reshape(n_runs, 2 * n_test), fit=fit)
