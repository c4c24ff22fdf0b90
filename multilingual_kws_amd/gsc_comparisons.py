"""The MSWC <-> GSC cross-comparison of the reference (notebooks/gsc_comparisons.py) against this build: the Speech-Commands split of
a keyword's clips, and cross_compare -- a five-shot model trained on one corpus, scored with model.evaluate on a test set of the same
corpus and on one of the other, each mixed with silence and unknown words.  The reference's home-directory paths are parameters here,
and the two accuracies are returned (and put on `q`, when one is given, as the reference's worker process did)."""
import glob
import hashlib
import os
import re
from dataclasses import dataclass
from typing import List

from .embedding import input_data
from .embedding import transfer_learning as tl

MAX_NUM_WAVS_PER_CLASS = 2 ** 27 - 1  # ~134M, the constant of Speech Commands' own split


def which_set(filename, validation_percentage, testing_percentage):
    """Speech Commands' stable split: "validation", "testing" or "training" from the SHA-1 of the file's base name with everything
    from "_nohash_" on removed, so that the recordings of one speaker stay together and a file never changes sets as others are added."""
    hash_name = re.sub(r"_nohash_.*$", "", os.path.basename(filename))
    hashed = hashlib.sha1(hash_name.encode("utf-8")).hexdigest()
    percentage_hash = (int(hashed, 16) % (MAX_NUM_WAVS_PER_CLASS + 1)) * (100.0 / MAX_NUM_WAVS_PER_CLASS)
    if percentage_hash < validation_percentage:
        return "validation"
    if percentage_hash < testing_percentage + validation_percentage:
        return "testing"
    return "training"


def load_gsc_data(keyword, gsc_dir, VAL_PCT=10, TEST_PCT=10):
    """gsc_dir: a Speech Commands directory (one sub-directory per word).  -> (train, validation, test) files of `keyword` by which_set,
    and the files of every other word (not _background_noise_) as the unknown pool; all four sorted."""
    gsc_dir = os.fspath(gsc_dir)
    kw_files = sorted(glob.glob(os.path.join(gsc_dir, keyword, "*.wav")))
    split = {"training": [], "validation": [], "testing": []}
    for f in kw_files:
        split[which_set(f, VAL_PCT, TEST_PCT)].append(f)
    others = [d for d in os.listdir(gsc_dir) if os.path.isdir(os.path.join(gsc_dir, d)) and d != keyword and d != "_background_noise_"]
    unknown = sorted(f for d in others for f in glob.glob(os.path.join(gsc_dir, d, "*.wav")))
    return split["training"], split["validation"], split["testing"], unknown


@dataclass(frozen=True)
class CrossCompare:
    keyword: str
    train_files: List[str]
    val_files: List[str]
    test_files: List[str]
    cross_testset: List[str]
    unknown_test: List[str]
    unknown_cross: List[str]
    verbose: int = 0


def evaluation_dataset(keyword, files, unknown_files, bg_datadir, model_settings=None, seed=0, batch_size=32):
    """The dataset cross_compare evaluates on: `files` labelled as the keyword, with silence (10 %) and unknown words (50 %) mixed in,
    in batches of 32, from an AudioDataset seeded with 0."""
    model_settings = model_settings or input_data.standard_microspeech_model_settings(3)
    audio_dataset = input_data.AudioDataset(model_settings=model_settings, commands=[keyword], background_data_dir=bg_datadir,
                                            unknown_files=unknown_files, unknown_percentage=50,
                                            spec_aug_params=input_data.SpecAugParams(percentage=80), seed=seed)
    return audio_dataset.eval_with_silence_unknown(input_data.AUTOTUNE, files, label_from_parent_dir=False).batch(batch_size)


def train(c, unknown_files, base_model_path, bg_datadir, model_settings, seed=None):
    """The reference's fine-tune for this comparison: 4 epochs, 2 batches of 32, head only, on the embedding cut at dense_2."""
    _, model, _ = tl.transfer_learn(
        target=c.keyword, train_files=c.train_files, val_files=c.val_files, unknown_files=unknown_files, num_epochs=4, num_batches=2,
        batch_size=32, primary_lr=0.001, backprop_into_embedding=False, embedding_lr=0, model_settings=model_settings,
        base_model_path=base_model_path, base_model_output="dense_2", bg_datadir=bg_datadir, csvlog_dest=None, verbose=c.verbose, seed=seed)
    return model


def cross_compare(c: CrossCompare, q=None, base_model_path="synthetic", unknown_files=(), bg_datadir=None, seed=None, return_model=False):
    """Trains on c.train_files (unknown_files: the unknown-word bank of the fine-tune), then model.evaluate on c.test_files mixed with
    c.unknown_test and on c.cross_testset mixed with c.unknown_cross.  -> (test_accuracy, cross_accuracy), also put on q when given;
    return_model=True appends the trained model.  seed: transfer_learn's (head initialisation and augmentation; None as the reference)."""
    model_settings = input_data.standard_microspeech_model_settings(3)
    model = train(c, list(unknown_files), base_model_path, bg_datadir, model_settings, seed)
    test_results = model.evaluate(evaluation_dataset(c.keyword, c.test_files, c.unknown_test, bg_datadir, model_settings))
    cross_results = model.evaluate(evaluation_dataset(c.keyword, c.cross_testset, c.unknown_cross, bg_datadir, model_settings))
    if c.verbose:
        print(test_results)
        print(cross_results)
    testacc_crossacc = (test_results[1], cross_results[1])
    if q is not None:
        q.put(testacc_crossacc)
    return testacc_crossacc + (model,) if return_model else testacc_crossacc
