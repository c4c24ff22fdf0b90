"""transfer_learning.transfer_learn_many: the argument checks that come before any device call (no GPU)."""
import pytest

from multilingual_kws_amd.embedding import input_data, transfer_learning as tl


def call(**over):
    kw = dict(targets=["a", "b"], train_files=[["a0.wav"], ["b0.wav"]], val_files=[["a1.wav"], ["b1.wav"]], unknown_files=[], num_epochs=1,
              num_batches=1, batch_size=4, primary_lr=1e-3, model_settings=input_data.standard_microspeech_model_settings(3),
              base_model_path="synthetic", bg_datadir=None, verbose=0)
    kw.update(over)
    return tl.transfer_learn_many(**kw)


@pytest.mark.parametrize("over", [
    dict(train_files=[["a0.wav"]]),
    dict(val_files=[["a1.wav"], ["b1.wav"], ["c1.wav"]]),
    dict(train_files={"a": ["a0.wav"]}),                    # a dict must name every target
    dict(train_files="a0.wav"),
    dict(seed=[1]),
    dict(seed=[1, 2, 3]),
    dict(csvlog_dest=["only_one.csv"]),
    dict(targets=[], train_files=[], val_files=[]),
], ids=["train_short", "val_long", "dict_missing", "not_per_target", "seed_short", "seed_long", "csv_short", "no_targets"])
def test_lengths_must_agree(over):
    with pytest.raises(ValueError):
        call(**over)


def test_duplicate_targets():
    with pytest.raises(ValueError, match="duplicate"):
        call(targets=["a", "a"])


def test_unknown_base_model_output():
    with pytest.raises(ValueError, match="base_model_output"):
        call(base_model_output="dense_7")


def test_side_by_side_must_be_positive():
    with pytest.raises(ValueError, match="side_by_side"):
        call(side_by_side=0)
