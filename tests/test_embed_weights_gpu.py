"""-m gpu: the embedding forward and the training step on weights CHOSEN TO TELL: every plan, every stage, on every set of
tests/util_embed_blobs.py -- non-trivial normalization, negative and small gammas, channels whose gain epsilon alone sets, gates in both
saturated tails, all of it at once.  tests/test_embed_blobs_cpu.py holds the float32 oracle ALONE to a third (forward) and a tenth (training
step) of the bounds below, on the same inputs: a case that fails here is a finding in the kernels or the wrappers, never in the reference.

Reference: the float64 oracle's 69 taps and embedding of the eight named clips, computed once per set from the very blob the handle is made of.
Handles: one default-option handle per plan class of tests/util_embed_plan.py at the class's smallest size (and 32, 256, 512, 1025), the seven
option combinations of test_execution_options_agree on 1024 clips, the multi-kernel and no-cluster plans of test_serving_handle_plans on 1 and 5
clips, the cluster kernel by option on 64 clips.  Batch: B = min(max_batch, 9), row r holds clip r % 8 (a plan follows the handle's size, not
B; nine clips fill two 4-clip workgroups or one 8-clip pair and leave a ragged one).
Asserted CLIP BY CLIP, one clip never sets another's scale: every tap and the embedding of the three noise clips within REL_TOL = 1e-4 of the
clip's own max |reference| and within the element-wise 1e-3 |b| + 1e-5 max |b| of _within; the five other clips within 1e-3; equal argmax;
everything finite; sub-batches bit-equal to the rows of the full batch.  Printed per case: the largest share of each bound, and where."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import util_embed_blobs as ub  # noqa: E402
import util_embed_plan as up  # noqa: E402
from test_embedding_gpu import REL_TOL  # noqa: E402

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

OTHER_TOL = 1e-3                  # the project's bound, for the silent, loud, corner and sparse clips
MAX_ROWS = 9
ALWAYS = (1, 2, 5, 32, 33, 256, 512, 1024, 1025)


def class_sizes(cus):
    """The smallest handle size of every plan class on a cus-CU device."""
    return [1] + [n for n, _ in up.boundaries(cus)]


# The parametrisation is that of a 256-CU device (MI355X); test_classes_only_another_cu_count_has adds what another device has besides.
SIZES_256 = sorted(set(class_sizes(256)) | set(ALWAYS))
# (front, block, mid, pair) of tests/test_embedding_gpu.py::test_execution_options_agree, in its order
COMBOS = ((0, 0, 0, 0), (1, 0, 0, 1), (1, 2, 1, 1), (0, 2, 0, 0), (1, 1, 2, 1), (0, 0, 1, 0), (1, 2, 1, 0))
CASES = ([(n, "default") for n in SIZES_256] + [(1024, "combo%d" % c) for c in range(len(COMBOS))]
         + [(n, plan) for n in (1, 5) for plan in ("multi-kernel", "no-cluster")] + [(64, "cluster")])


def _set_options(em, how):
    """-> False when the dispatch probe turned off what the case is about."""
    if how == "multi-kernel":
        for k in ("fuse_block", "fuse_mid", "fuse_back", "fuse_pair", "fuse_cluster"):
            em.set_option(k, 0)
    elif how == "no-cluster":
        em.set_option("fuse_cluster", 0)
    elif how == "cluster":
        if em.get_option("fuse_pair") != 1:
            return False
        em.set_option("fuse_cluster", 1)
    elif how.startswith("combo"):
        combo = int(how[5:])
        front, block, mid, pair = COMBOS[combo]
        for k, v in (("fuse_chain", combo & 1), ("fuse_pair", pair), ("fuse_front", front), ("fuse_block", block), ("fuse_mid", mid),
                     ("fuse_walk", (combo >> 1) & 1), ("fuse_se4", (combo >> 2) & 1), ("fuse_back", 1 if mid != 2 else 0),
                     ("fuse_stem", front), ("fuse_gap", front)):
            em.set_option(k, v)
    else:
        assert how == "default"
    return True


@pytest.fixture(scope="module")
def dev():
    d = torch.device("cuda:0")
    return dict(dev=d, cus=torch.cuda.get_device_properties(d).multi_processor_count,
                x=torch.from_numpy(ub.clips()[np.arange(MAX_ROWS) % 8].copy()).to(d))


def _shares(got, ref, clip):
    """Shares of the bounds one row uses against the float64 reference of its clip: {bound name: share}."""
    got = got.astype(np.float64)
    err, top = np.abs(got - ref), float(np.abs(ref).max())
    if clip in ub.NOISE:
        return {"noise 1e-4": float(err.max()) / top / REL_TOL, "noise element-wise": float((err / (1e-3 * np.abs(ref) + 1e-5 * top)).max())}
    return {"other 1e-3": float(err.max()) / top / OTHER_TOL}


def _check_case(dev, name, n, how):
    from multilingual_kws_amd.embedding_model import EmbeddingModel
    ref_emb, ref_taps = ub.reference(name)
    B = min(n, MAX_ROWS)
    x = dev["x"][:B]
    em = EmbeddingModel(ub.blob(name), max_batch=n)
    try:
        if not _set_options(em, how):
            pytest.skip("dispatch probe failed on this device: the cluster kernel is not in use")
        full = em.forward(x)
        got = {t: em.tap(x, t).cpu().numpy().reshape(B, -1) for t in ref_taps}
        got["embedding"] = full.cpu().numpy()
        worst, failed = {}, []
        for t, g in got.items():
            ref = ref_emb if t == "embedding" else ref_taps[t]
            assert g.shape == (B, ref.shape[1]), (name, n, how, t, g.shape)
            assert np.isfinite(g).all(), (name, n, how, t)
            for r in range(B):
                for bound, share in _shares(g[r], ref[r % 8], r % 8).items():
                    if share > worst.get(bound, (0.0,))[0]:
                        worst[bound] = (share, t, r)
                    if not share < 1.0:
                        failed.append((t, r, ub.CLIP_NAMES[r % 8], bound, share))
        print("%s, %d clips, %s: largest share of each bound: " % (name, n, how)
              + "; ".join("%s %.3f (%s, row %d)" % ((b,) + worst[b]) for b in sorted(worst)))
        assert not failed, (name, n, how, "first failing taps in network order", failed[:6])
        assert np.array_equal(got["embedding"].argmax(1), ref_emb[np.arange(B) % 8].argmax(1)), (name, n, how)
        for b in sorted({b for b in (1, 2, 3, B // 2 + 1, B - 3, B - 1) if 1 <= b < B}):
            assert torch.equal(em.forward(x[:b]), full[:b]), (name, n, how, b)
    finally:
        em.close()


@pytest.mark.parametrize("n,how", CASES, ids=["%d-%s" % c for c in CASES])
@pytest.mark.parametrize("name", ub.SETS)
def test_every_stage_on_every_set(dev, name, n, how):
    if how == "default":
        assert n in class_sizes(256) or n in ALWAYS
    _check_case(dev, name, n, how)


@pytest.mark.parametrize("name", ub.SETS)
def test_classes_only_another_cu_count_has(dev, name):
    for n in class_sizes(dev["cus"]):
        if n not in SIZES_256:
            _check_case(dev, name, n, "default")


def test_predict_keeps_the_normalization(dev):
    """EmbeddingModel.predict on `normalized`: bit-equal to forward, and not what a handle of the same weights with mean 0 / variance 1 returns
    -- a wrapper or a handle that drops the normalization shows here."""
    from multilingual_kws_amd.embedding_model import EmbeddingModel
    spec = np.array(ub.clips())
    em, twin = EmbeddingModel(ub.blob("normalized"), max_batch=8), EmbeddingModel(ub.twin("normalized"), max_batch=8)
    try:
        out = em.predict(spec[..., None])
        assert out.shape == (8, 1024) and np.array_equal(out, em.forward(dev["x"][:8]).cpu().numpy())
        ref = ub.reference("normalized")[0]
        assert max(_shares(out[r], ref[r], r).get("noise 1e-4", 0.0) for r in range(8)) < 1.0
        other = twin.predict(spec[..., None])
        for r in range(8):
            assert np.abs(other[r] - out[r]).max() > 100 * REL_TOL * np.abs(ref[r]).max(), ub.CLIP_NAMES[r]
    finally:
        em.close()
        twin.close()


def _train_step(blob):
    from multilingual_kws_amd.embedding_trainer import EmbeddingTrainer
    spec, proj, masks = ub.train_inputs()
    tr = EmbeddingTrainer(blob)
    emb = tr.forward_train(torch.from_numpy(np.array(spec)).cuda(), masks)
    tr.backward(torch.from_numpy(np.tile(proj.astype(np.float32), (spec.shape[0], 1))).cuda())
    return tr, emb.cpu().numpy(), tr.named_grads()


@pytest.mark.parametrize("name", ub.TRAIN_SETS)
def test_training_step_on_telling_weights(name):
    """EmbeddingTrainer against the float64 TrainableEmbeddingOracle with the inputs and masks, and at the bounds, of
    tests/test_train_gpu.py::test_training_mode_gradients_match_the_oracle."""
    ref = ub.train_reference64(name)
    tr, emb, got = _train_step(ub.blob(name))
    e = float(np.abs(emb - ref["emb"]).max() / np.abs(ref["emb"]).max())
    print("%s: training-mode embedding %.3g of its bound 1e-4" % (name, e / 1e-4))
    assert e < 1e-4, (name, e)
    gmax = max(float(np.abs(g).max()) for g in ref["grads"].values())
    share = {k: float(np.abs(got[k].reshape(g.shape).astype(np.float64) - g).max()) / ub.gradient_bound(g, gmax) for k, g in ref["grads"].items()}
    assert len(share) == len(ref["trainable"])
    order = sorted(share, key=share.get, reverse=True)
    print("%s: largest shares of the gradient bound: " % name + "; ".join("%s %.3f" % (k, share[k]) for k in order[:3]) + "; gmax %.3g" % gmax)
    assert share[order[0]] <= 1.0, (name, [(k, share[k]) for k in order if share[k] > 1.0])
    frozen = [k for k in got if k not in ref["grads"]]
    assert len(frozen) == 2 + len(ref["moving"])
    for k in frozen:
        assert not got[k].any(), (name, k)                                  # non-trainable: exactly zero
    newp = tr.blob()
    moving = {}
    for k, val in ref["moving"].items():
        t = tr.tensors[k]
        moving[k] = float(np.abs(newp[t["offset"]:t["offset"] + t["count"]] - val).max() / np.abs(val).max())
    k = max(moving, key=moving.get)
    print("%s: new moving statistics %.3g of their bound 1e-5 (%s)" % (name, moving[k] / 1e-5, k))
    assert moving[k] < 1e-5, (name, k, moving[k])
    if name == "normalized":
        # a trainer that reads the two normalization tensors wrongly computes the twin's stem gradient
        _, _, twin = _train_step(ub.twin(name))
        g = ref["grads"]["stem_conv/kernel"]
        d = float(np.abs(twin["stem_conv/kernel"].reshape(g.shape) - got["stem_conv/kernel"].reshape(g.shape)).max())
        print("normalized: stem_conv/kernel gradient differs from the mean-0 / variance-1 twin's by %.3g, bound %.3g" % (d, ub.gradient_bound(g, gmax)))
        assert d > ub.gradient_bound(g, gmax)
