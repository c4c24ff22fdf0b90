"""-m gpu: transfer_learning.transfer_learn_many (K keyword heads trained side by side on one frozen embedding) against one
transfer_learn call per keyword with the same seeds: the same bits, the same history, name and details.

Three tiny synthetic keyword sets that share one unknown list and one background directory; FORWARD_CLIPS = 24 with 4-clip batches
and 2 epochs of 16 steps gives groups of 6, 6 and a cut group of 4 per epoch (as test_finetune_gpu's grouping test), and 6 steps per
forward is above OVERLAP_FROM_GROUP, so the default runs use the second stream."""
import contextlib

import numpy as np
import pytest

from tests.util_data import make_fewshot_dataset

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

TARGETS = ["alpha", "beta", "gamma"]
SEEDS = [5, 6, 7]


@contextlib.contextmanager
def patched(**attrs):
    from multilingual_kws_amd.embedding import transfer_learning as tl
    old = {k: getattr(tl, k) for k in attrs}
    try:
        for k, v in attrs.items():
            setattr(tl, k, v)
        yield tl
    finally:
        for k, v in old.items():
            setattr(tl, k, v)


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    sets = [make_fewshot_dataset(str(tmp_path_factory.mktemp("kw%d" % i)), n_unknown=16 if i == 0 else 1, seed=i) for i in range(3)]
    return dict(train=[s["train"] for s in sets], val=[s["val"] for s in sets], unknown=sets[0]["unknown"], bg_dir=sets[0]["bg_dir"])


def common(data):
    from multilingual_kws_amd.embedding import input_data
    return dict(unknown_files=data["unknown"], num_epochs=2, num_batches=4, batch_size=4, primary_lr=1e-3,
                model_settings=input_data.standard_microspeech_model_settings(3), base_model_path="synthetic", base_model_output="dense_2",
                bg_datadir=data["bg_dir"], verbose=0)


def summary(result):
    name, model, details = result
    return name, details, model.history, model.head.get_params()


def assert_same(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g[0] == w[0] and g[1] == w[1] and g[2] == w[2], (g[:3], w[:3])
        assert np.array_equal(g[3], w[3])


@pytest.fixture(scope="module")
def singles(data):
    """The reference: one transfer_learn call per keyword (computed once, compared by every test)."""
    with patched(FORWARD_CLIPS=24) as tl:
        return [summary(tl.transfer_learn(TARGETS[i], data["train"][i], data["val"][i], backprop_into_embedding=False, embedding_lr=0,
                                          seed=SEEDS[i], **common(data))) for i in range(3)]


def test_side_by_side_equals_one_call_per_keyword(data, singles):
    seen_g, seen_overlap = [], []
    with patched(FORWARD_CLIPS=24) as tl:
        real_refill, real_init = tl.FrozenHeadGroupTrainer._refill, tl.FrozenHeadGroupTrainer.__init__

        def refill(self, g):
            seen_g.append(g)
            return real_refill(self, g)

        def init(self, *a, **k):
            real_init(self, *a, **k)
            seen_overlap.append((self.K, self.overlap))
        tl.FrozenHeadGroupTrainer._refill, tl.FrozenHeadGroupTrainer.__init__ = refill, init
        try:
            results = tl.transfer_learn_many(TARGETS, data["train"], dict(zip(TARGETS, data["val"])), seed=SEEDS, side_by_side=3, **common(data))
        finally:
            tl.FrozenHeadGroupTrainer._refill, tl.FrozenHeadGroupTrainer.__init__ = real_refill, real_init
    assert seen_g == [6, 6, 4, 6, 6, 4] and seen_overlap == [(3, True)]
    assert_same([summary(r) for r in results], singles)
    assert [r[2]["target"] for r in results] == TARGETS and len({s[0] for s in singles}) == 3
    assert len({tuple(s[3]) for s in singles}) == 3                 # three different heads
    # one shared embedding; the heads are ordinary serving heads
    from multilingual_kws_amd.head import Head
    models = [r[1] for r in results]
    assert all(m.embedding is models[0].embedding for m in models)
    emb = models[0].embedding.forward(torch.zeros((5, 49, 40), device=models[0].embedding.device))
    many = Head.forward_many([m.head for m in models], emb)
    assert many.shape == (3, 5, 3)
    assert torch.equal(many, torch.stack([m.head.forward(emb) for m in models]))
    assert [m.head.step_t for m in models] == [32] * 3


def test_waves_and_integer_seed(data, singles, tmp_path):
    """side_by_side = 2: waves of two and one; seed = 5 means 5, 6, 7; the CSV logs are written per target."""
    csvs = [str(tmp_path / ("%s.csv" % t)) for t in TARGETS]
    with patched(FORWARD_CLIPS=24) as tl:
        results = tl.transfer_learn_many(TARGETS, data["train"], data["val"], seed=5, side_by_side=2, csvlog_dest=csvs, **common(data))
    assert_same([summary(r) for r in results], singles)
    assert results[0][1].embedding is results[2][1].embedding
    for path, s in zip(csvs, singles):
        rows = open(path).read().split()
        assert rows[0] == "epoch,accuracy,loss,val_accuracy,val_loss" and len(rows) == 3
        assert float(rows[2].split(",")[3]) == s[2]["val_accuracy"][1]


def test_second_stream_changes_no_bit(data, singles):
    seen = []
    with patched(FORWARD_CLIPS=24, OVERLAP_FROM_GROUP=1000) as tl:
        real_init = tl.FrozenHeadGroupTrainer.__init__

        def init(self, *a, **k):
            real_init(self, *a, **k)
            seen.append(self.overlap)
        tl.FrozenHeadGroupTrainer.__init__ = init
        try:
            results = tl.transfer_learn_many(TARGETS, data["train"], data["val"], seed=SEEDS, **common(data))
        finally:
            tl.FrozenHeadGroupTrainer.__init__ = real_init
    assert seen == [False]
    assert_same([summary(r) for r in results], singles)      # the singles and the first test ran with the second stream on
