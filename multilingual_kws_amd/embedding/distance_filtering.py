"""Embedding consumers of the hot path, same names and return contracts as the reference:

* embedding_model / cluster_and_sort      -- multilingual_kws/embedding/distance_filtering.py:12-83
* embed_files / export_keyword_embeddings -- notebooks/dataperf_experiments.py:320-338,385-415 (DataPerf export:
  one parquet per keyword with columns clip_id, mswc_embedding_vector)

Spectrograms and feature vectors come from the HIP path (one frontend launch + one embedding pass per batch
of up to 1024 clips instead of a per-file TF op); k-means stays sklearn.cluster.KMeans with the reference's
arguments, so given equal feature vectors the clustering is the reference's.  cluster_and_sort_many is the K-keyword form: the
clustering and the distances run on the device (multilingual_kws_amd/kmeans.py holds the restatement of that KMeans call).
"""
import os
from pathlib import Path

import numpy as np

from . import input_data
from .transfer_learning import _specs_for_files, load_base_model


def embedding_model(base_model_path="synthetic", base_model_output="dense_2", max_batch=1024):
    """distance_filtering.py:12-28.  Returns the frozen embedding with a Keras-style .predict([N,49,40(,1)]) ->
    [N,1024].  base_model_path: weight-container directory (multilingual_kws_amd.weights.save) or "synthetic[:seed]"."""
    if base_model_output != "dense_2":
        raise NotImplementedError("the embedding is cut at dense_2 (the layer every reference call site uses)")
    model, _ = load_base_model(base_model_path, max_batch=max_batch)
    return model


def embed_files(files, embedding, model_settings=None, batch_size=1024, convert=False):
    """dataperf_experiments.py:320-338: list of WAV paths -> float32 [N, 1024], in batches of `batch_size`.  convert=True: the files may
    have any supported format, rate and channel count (input_data.read_clips: channel 0, decoded and converted on the device)."""
    if model_settings is None:
        model_settings = input_data.standard_microspeech_model_settings(label_count=3)
    files = [str(f) for f in files]
    out = np.zeros((len(files), 1024), dtype=np.float32)
    for s in range(0, len(files), batch_size):
        chunk = files[s:s + batch_size]
        out[s:s + len(chunk)] = embedding.predict(_specs_for_files(chunk, model_settings, convert=True) if convert else _specs_for_files(chunk, model_settings))
    return out


def cluster_and_sort(keyword_samples, embedding_model, seed=123, n_train=50, n_clusters=5, model_settings=None):
    """distance_filtering.py:30-83.
    Returns:
        dict(sorted_clips, cluster_centers, distances, train_clips): evaluation clips sorted by the L2 distance to
        their closest k-means centre (k-means fitted on the embeddings of n_train randomly chosen clips).
    """
    import sklearn.cluster
    if model_settings is None:
        model_settings = input_data.standard_microspeech_model_settings(label_count=761)
    assert len(keyword_samples) > n_train, f"{n_train} > number of keyword samples"

    rng = np.random.RandomState(seed)
    kwdata = rng.permutation(keyword_samples)
    train_clips = kwdata[:n_train]
    eval_clips = kwdata[n_train:]

    feature_vectors = embed_files(train_clips, embedding_model, model_settings)
    kmeans = sklearn.cluster.KMeans(n_clusters=n_clusters, random_state=seed).fit(feature_vectors)
    eval_vectors = embed_files(eval_clips, embedding_model, model_settings)

    l2_distances = np.linalg.norm(kmeans.cluster_centers_[np.newaxis].astype(np.float32) - eval_vectors[:, np.newaxis], axis=-1)
    l2_from_closest_cluster = l2_distances.min(axis=1)
    sorting = np.argsort(l2_from_closest_cluster)
    return dict(
        sorted_clips=eval_clips[sorting],
        cluster_centers=kmeans.cluster_centers_,
        distances=l2_from_closest_cluster[sorting],
        train_clips=train_clips,
    )


TRAIN_EMBEDDING_BYTES = 256 << 20     # cluster_and_sort_many: train embeddings retained on the device per chunk of keywords


def _result(eval_clips, train_clips, centers, dist, which, labels, n_iter, fallback):
    sorting = np.argsort(dist)                                       # on the host, as in the reference: ties behave the same
    return dict(sorted_clips=eval_clips[sorting], cluster_centers=centers, distances=dist[sorting], train_clips=train_clips,
                labels=labels, n_iter=int(n_iter), nearest=which[sorting], fallback=bool(fallback))


def _sklearn_fit(vectors, n_clusters, seed):
    """The reference's own call, for a keyword whose Lloyd run met an empty cluster (not restated: multilingual_kws_amd/kmeans.py)."""
    import sklearn.cluster
    km = sklearn.cluster.KMeans(n_clusters=n_clusters, random_state=seed).fit(vectors)
    return km.cluster_centers_.astype(np.float32), km.labels_.astype(np.int32), int(km.n_iter_)


def _spec_batches(files, embedding, model_settings, convert=False):
    """Decode and featurise `files` in batches of the handle's max_batch: yields (first row, CUDA spectrograms)."""
    import torch
    n_samples, mb = model_settings["desired_samples"], embedding.max_batch
    for s in range(0, len(files), mb):
        if convert:
            audio = input_data.read_clips(files[s:s + mb], model_settings["sample_rate"], n_samples, device=embedding.device)
            yield s, input_data.to_micro_spectrogram(model_settings, audio)
            continue
        audio = np.stack([input_data._read_wav(f, n_samples) for f in files[s:s + mb]])
        yield s, input_data.to_micro_spectrogram(model_settings, torch.from_numpy(audio).to(embedding.device))


def cluster_and_sort_many(keyword_samples, embedding_model, seed=123, n_train=50, n_clusters=5, model_settings=None, convert=False):
    """cluster_and_sort for K keywords on one embedding handle.  keyword_samples: K lists of paths; seed: an int or K ints.
    -> K dicts: the four keys of cluster_and_sort with the same types (sorted_clips, cluster_centers float32 [n_clusters, 1024],
    distances float32, train_clips) and labels (of the train clips), n_iter, nearest (the centre each eval clip is nearest to, in sorted
    order), fallback (True where a Lloyd step met an empty cluster and the keyword went through the sklearn call).

    Every keyword is split by RandomState(seed).permutation, as in the reference.  The train clips of a chunk of keywords are embedded
    in batches of the handle's max_batch and stay on the device (at most TRAIN_EMBEDDING_BYTES of them: that bounds the chunk), one
    mkws_kmeans_fit clusters the chunk (multilingual_kws_amd/kmeans.py: kmeans_host is the specification, held to sklearn), and
    mkws_kmeans_nearest runs on every batch of eval embeddings while it is on the device: no eval embedding is retained or copied, 8
    bytes per eval clip come back.  The distance is (float32) sqrt(sum((float64)centre - (float64)x)^2) against the float32 centres.
    An embedding_model without a device `forward`, or a host without a GPU, takes the same flow through `predict` and kmeans_host.
    convert=True: the clips may have any supported format, rate and channel count (input_data.read_clips, channel 0)."""
    import torch
    from .. import kmeans
    if model_settings is None:
        model_settings = input_data.standard_microspeech_model_settings(label_count=761)
    keyword_samples = list(keyword_samples)
    K = len(keyword_samples)
    seeds = [int(seed)] * K if np.ndim(seed) == 0 else [int(s) for s in seed]
    if len(seeds) != K:
        raise ValueError(f"{len(seeds)} seeds for {K} keywords")
    train, evals = [], []
    for k, samples in enumerate(keyword_samples):
        assert len(samples) > n_train, f"{n_train} > number of keyword samples (keyword {k})"
        kwdata = np.random.RandomState(seeds[k]).permutation(samples)
        train.append(kwdata[:n_train])
        evals.append(kwdata[n_train:])
    if K == 0:
        return []

    if not (hasattr(embedding_model, "forward") and torch.cuda.is_available()):
        results = []
        for k in range(K):
            vectors = embed_files(train[k], embedding_model, model_settings, convert=convert)
            fit = kmeans.kmeans_host(vectors, n_clusters, seeds[k])
            if fit.empty:
                centers, labels, n_iter = _sklearn_fit(vectors, n_clusters, seeds[k])
            else:
                centers, labels, n_iter = fit.centers.astype(np.float32), fit.labels, fit.n_iter
            dist, which = kmeans.nearest_host(embed_files(evals[k], embedding_model, model_settings, convert=convert), centers)
            results.append(_result(evals[k], train[k], centers, dist, which, labels, n_iter, fit.empty))
        return results

    dim, dev = embedding_model.output_dim, embedding_model.device
    kmeans.check_groups([0, n_train], n_train, dim, n_clusters)      # refused before anything is decoded
    per_chunk = max(1, TRAIN_EMBEDDING_BYTES // (n_train * dim * 4))
    results = []
    for k0 in range(0, K, per_chunk):
        ks = range(k0, min(K, k0 + per_chunk))
        G = len(ks)
        train_files = [str(f) for k in ks for f in train[k]]
        eval_files = [str(f) for k in ks for f in evals[k]]
        group = np.concatenate([np.full(len(evals[k]), g, np.int32) for g, k in enumerate(ks)])
        offsets = np.arange(G + 1, dtype=np.int64) * n_train
        with torch.cuda.device(dev):
            d_train = torch.empty((len(train_files), dim), dtype=torch.float32, device=dev)

            def fit_pass():
                for s, spec in _spec_batches(train_files, embedding_model, model_settings, convert):
                    embedding_model.forward(spec, out=d_train[s:s + spec.shape[0]])
                return kmeans.kmeans_fit_on_device(d_train, offsets, n_clusters, [seeds[k] for k in ks])     # ends in the copy back

            fit = embedding_model.checked(fit_pass)
            centers, labels, n_iter = fit.centers.copy(), fit.labels.reshape(G, n_train).copy(), fit.info[:, 1].copy()
            fell_back = fit.info[:, 0] != 0
            for g in np.nonzero(fell_back)[0]:
                vectors = d_train[g * n_train:(g + 1) * n_train].cpu().numpy()
                centers[g], labels[g], n_iter[g] = _sklearn_fit(vectors, n_clusters, seeds[ks[g]])
                fit.d_centers[g].copy_(torch.from_numpy(centers[g]))
            del d_train
            mb = embedding_model.max_batch
            n_eval, n_batches = len(eval_files), (len(eval_files) + mb - 1) // mb
            d_group = torch.from_numpy(group).to(dev)

            def eval_pass():
                d_emb = torch.empty((min(mb, n_eval), dim), dtype=torch.float32, device=dev)
                d_out = torch.empty(2 * n_eval + n_batches, dtype=torch.int32, device=dev)     # distances, indices, a counter per batch
                d_dist, d_which = d_out[:n_eval].view(torch.float32), d_out[n_eval:2 * n_eval]
                for b, (s, spec) in enumerate(_spec_batches(eval_files, embedding_model, model_settings, convert)):
                    r = spec.shape[0]
                    embedding_model.forward(spec, out=d_emb[:r])
                    kmeans.nearest_on_device(d_emb[:r], d_group[s:s + r], fit.d_centers,
                                             out=(d_dist[s:s + r], d_which[s:s + r], d_out[2 * n_eval + b:2 * n_eval + b + 1]))
                return d_out.cpu().numpy()

            out = embedding_model.checked(eval_pass)
        if out[2 * n_eval:].any():
            raise RuntimeError("eval clips with a keyword outside the chunk reached the device")
        dist, which = out[:n_eval].view(np.float32), out[n_eval:2 * n_eval]
        at = 0
        for g, k in enumerate(ks):
            m = len(evals[k])
            results.append(_result(evals[k], train[k], centers[g], dist[at:at + m], which[at:at + m], labels[g], n_iter[g], fell_back[g]))
            at += m
    return results


def export_keyword_embeddings(clips_dir, dest_dir, embedding, model_settings=None, batch_size=1024, keywords=None, convert=False):
    """dataperf_experiments.py:385-415: for every keyword directory under clips_dir write
    dest_dir/<keyword>.parquet with columns clip_id (path relative to clips_dir) and mswc_embedding_vector.
    Existing parquets are skipped (resume) and so are empty keyword directories, as in the reference loop.
    Returns the list of files written.  convert: embed_files' switch."""
    import pandas as pd
    clips_dir, dest_dir = Path(clips_dir), Path(dest_dir)
    dest_dir.mkdir(parents=True, exist_ok=True)
    if keywords is None:
        keywords = list(sorted(os.listdir(clips_dir)))
    written = []
    for keyword in keywords:
        keyword_samples = list(sorted((clips_dir / keyword).glob("*.wav")))
        dest = dest_dir / f"{keyword}.parquet"
        if dest.exists() or len(keyword_samples) == 0:
            continue
        feature_vecs = embed_files(keyword_samples, embedding, model_settings, batch_size, convert=convert)
        id_paths = [str(fp.relative_to(clips_dir)) for fp in keyword_samples]
        df = pd.DataFrame(data=dict(clip_id=id_paths, mswc_embedding_vector=pd.Series(list(feature_vecs))))
        df.to_parquet(dest)
        written.append(dest)
    return written
