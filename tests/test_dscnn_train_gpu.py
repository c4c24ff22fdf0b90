"""-m gpu: the DS-CNN training operators (mkws_op_dscnn_*, mkws_op_dropout_*), the tape of dscnn_trainer.DSCNNTrainer and
dscnn_comparison.train against the float64 oracle of tests/dscnn_train_cases.py.  The whole-step batches are functions of the launch
constants the library reports (mkws_op_get_option), so a retune of a route moves the cases along with it.

ReLU kinks: a gradient through a ReLU is discontinuous where the pre-activation is zero, and among up to 3.2 M cells a layer some
pre-activation always lies closer to zero than float32 resolves.  Measured with the plain oracle: at B = 20, 32, 33, 65, 100 one or two
cells, all with |pre-activation| <= 1e-5, came out on the other side than in float64, and one such cell moved gradients by up to 7e-3 of
max |reference| (B = 32; 1e-6..1.5e-5 without).  The oracle therefore takes the side of cells within 1e-5 of zero from the device's
activations (_oracle_step); everywhere else the sides must agree.  Bounds and cases are as they were."""
import os

import numpy as np
import pytest

from multilingual_kws_amd import dscnn, dscnn_comparison, dscnn_trainer, synth
from tests import dscnn_cases
from tests import dscnn_train_cases as cases
from tests.util_train_ops import make_ops

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
F = torch.nn.functional
PIX = 500


def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-300))


@pytest.fixture(scope="module")
def ops():
    o = make_ops()
    o.step = torch.zeros(1, dtype=torch.int32, device=o.dev)
    return o


@pytest.fixture(autouse=True)
def _arena(ops):
    ops.check(ops.L.mkws_train_ctx_bind(None))
    ops.check(ops.L.mkws_op_set_scratch(ops.p(ops.scratch), ops.scratch.numel()))
    ops.step.zero_()


def _option(ops, name):
    v = ops.L.mkws_op_get_option(name.encode())
    assert v > 0, name
    return v


def _new(ops, *shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device=ops.dev)


# ---- stem ---------------------------------------------------------------------------------------------------------------------------
STEM_BATCHES = (1, 2, 3, 67)


def _stem_inputs(case):
    if case == "deterministic":
        return dscnn_cases.deterministic_clips()[0]
    return np.asarray(cases.clips(67)[:case])


def _stem_reference(spec, kernel):
    x = F.pad(torch.from_numpy(spec.astype(np.float64))[:, None], (1, 1, 4, 5))
    w = torch.from_numpy(kernel.astype(np.float64)).permute(3, 2, 0, 1).clone().requires_grad_(True)
    z = F.conv2d(x, w, stride=2)
    return z, w


@pytest.mark.parametrize("case", STEM_BATCHES + ("deterministic",))
def test_stem_forward(ops, case):
    spec = _stem_inputs(case)
    kernel = dscnn.unpack(cases.params())["conv2d/kernel"]
    B = spec.shape[0]
    Z, d_spec, d_kernel = _new(ops, B, 25, 20, 64), ops.t(spec), ops.t(kernel)
    ops.check(ops.L.mkws_op_dscnn_stem_fwd(ops.p(d_spec), ops.p(d_kernel), ops.p(Z), B, ops.s()))
    want = _stem_reference(spec, kernel)[0].detach().permute(0, 2, 3, 1).numpy()
    got = Z.cpu().numpy()
    assert _rel(got, want) <= 1e-5
    if case == "deterministic":          # clip by clip: the full-scale clip must not hide the impulses (the all-zero clip gives exact zeros)
        for b in range(B):
            assert np.abs(got[b] - want[b]).max() <= 1e-5 * np.abs(want[b]).max(), b


@pytest.mark.parametrize("case", STEM_BATCHES + ("deterministic",))
def test_stem_weight_gradient(ops, case):
    spec = _stem_inputs(case)
    kernel = dscnn.unpack(cases.params())["conv2d/kernel"]
    B = spec.shape[0]
    dZ = np.random.default_rng(B).standard_normal((B, 25, 20, 64)).astype(np.float32)
    z, w = _stem_reference(spec, kernel)
    (z * torch.from_numpy(dZ.astype(np.float64)).permute(0, 3, 1, 2)).sum().backward()
    want = w.grad.permute(2, 3, 1, 0).numpy().reshape(40, 64)
    d_spec, d_dZ = ops.t(spec), ops.t(dZ)
    runs = []
    for _ in range(2):
        dW = _new(ops, 40, 64)
        ops.check(ops.L.mkws_op_dscnn_stem_bwd_weight(ops.p(d_spec), ops.p(d_dZ), ops.p(dW), B, ops.s()))
        runs.append(dW.cpu().numpy())
    assert _rel(runs[0], want) <= 1e-4
    assert np.array_equal(runs[0].view(np.uint32), runs[1].view(np.uint32))


# ---- dropout ------------------------------------------------------------------------------------------------------------------------
def _dropout_sizes(ops):
    cap = _option(ops, "grid_cap")
    return {"one": (1, 0), "seven": (7, 0), "vector-grid-stride": (cap * 256 * 4 + 4 * 256 + 3, 0), "unaligned-grid-stride": (cap * 256 + 5, 1)}


@pytest.mark.parametrize("size", ("one", "seven", "vector-grid-stride", "unaligned-grid-stride"))
def test_dropout(ops, size):
    n, offset = _dropout_sizes(ops)[size]
    cap = _option(ops, "grid_cap")
    if size == "vector-grid-stride":
        assert n % 4 != 0 and n // 4 > cap * 256
    if size == "unaligned-grid-stride":
        assert n > cap * 256
    seed, site, rate, step = 77, 3, 0.2, 5
    ops.step.fill_(step)
    x = torch.from_numpy(np.random.default_rng(1).standard_normal(n + offset).astype(np.float32)).to(ops.dev)[offset:]
    assert (x.data_ptr() % 16 == 0) == (offset == 0)
    mask = dscnn_trainer.dropout_mask_host(seed, step, site, n, rate)
    scale = dscnn_trainer.dropout_scale(rate)
    want = np.where(mask, x.cpu().numpy() * scale, np.float32(0)).astype(np.float32)
    out = torch.full((n + offset,), float("nan"), dtype=torch.float32, device=ops.dev)[offset:]
    ops.check(ops.L.mkws_op_dropout_fwd(ops.p(x), ops.p(out), n, rate, seed, ops.p(ops.step), site, ops.s()))
    assert np.array_equal(out.cpu().numpy().view(np.uint32), want.view(np.uint32))
    # backward: the same mask on the gradient, in place
    g = x.clone()
    ops.check(ops.L.mkws_op_dropout_bwd(ops.p(g), ops.p(g), n, rate, seed, ops.p(ops.step), site, ops.s()))
    assert np.array_equal(g.cpu().numpy().view(np.uint32), want.view(np.uint32))
    # rate 0 is the identity
    ops.check(ops.L.mkws_op_dropout_fwd(ops.p(x), ops.p(out), n, 0.0, seed, ops.p(ops.step), site, ops.s()))
    assert torch.equal(out, x)
    if n >= 7:                           # another step, another mask (and the host twin follows)
        ops.step.fill_(step + 1)
        ops.check(ops.L.mkws_op_dropout_fwd(ops.p(x), ops.p(out), n, rate, seed, ops.p(ops.step), site, ops.s()))
        kept = out.cpu().numpy() != 0
        assert np.array_equal(kept, dscnn_trainer.dropout_mask_host(seed, step + 1, site, n, rate) & (x.cpu().numpy() != 0))
        assert n < 100 or not np.array_equal(kept, mask & (x.cpu().numpy() != 0))


def test_dropout_refuses_bad_rates(ops):
    x = _new(ops, 8)
    for rate in (1.0, -0.1):
        assert ops.L.mkws_op_dropout_fwd(ops.p(x), ops.p(x), 8, rate, 1, ops.p(ops.step), 0, ops.s()) < 0


# ---- pool ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", (1, 5))
def test_pool(ops, B):
    seed, site, rate, step = 9, 1, 0.4, 2
    ops.step.fill_(step)
    A = np.abs(np.random.default_rng(B).standard_normal((B, 25, 20, 64))).astype(np.float32)
    mask = dscnn_trainer.dropout_mask_host(seed, step, site, A.size, rate).reshape(A.shape)
    scale = dscnn_trainer.dropout_scale(rate)
    want = (A.astype(np.float64) * mask)[:, :24].sum(axis=(1, 2)) * float(scale) / 480.0
    pooled, d_A = _new(ops, B, 64), ops.t(A)
    ops.check(ops.L.mkws_op_dscnn_pool_fwd(ops.p(d_A), B, rate, seed, ops.p(ops.step), site, ops.p(pooled), ops.s()))
    assert _rel(pooled.cpu().numpy(), want) <= 1e-6
    dp = np.random.default_rng(B + 10).standard_normal((B, 64)).astype(np.float32)
    dA, d_dp = _new(ops, B, 25, 20, 64), ops.t(dp)
    ops.check(ops.L.mkws_op_dscnn_pool_bwd(ops.p(d_dp), B, rate, seed, ops.p(ops.step), site, ops.p(dA), ops.s()))
    got = dA.cpu().numpy()
    assert not got[:, 24].any() and not np.signbit(got[:, 24]).any()
    gscale = np.float32(scale / np.float32(480.0))
    want_rows = np.where(mask[:, :24], (dp * gscale)[:, None, None, :], np.float32(0)).astype(np.float32)
    assert np.array_equal(got[:, :24].view(np.uint32), want_rows.view(np.uint32))


# ---- one whole step -------------------------------------------------------------------------------------------------------------------
MASK_SEED = 21
ROUTES = {"one": None, "bn_small_rows": 1, "bn_max_gemm_tiles": 64, "bn_chunk_cap": 128, "bn_max_chunks": 128, "reference-batch": None}


def _route_batches(ops):
    """{case: B}: both sides of every row-count boundary the step crosses, B = 1 and the reference's batch of 100."""
    out = {"one": 1, "reference-batch": 100}
    for name, rows_per in ROUTES.items():
        if rows_per is None:
            continue
        rows = _option(ops, name) * rows_per
        b = rows // PIX
        assert b >= 1 and b * PIX <= rows < (b + 1) * PIX
        out[name + "-below"], out[name + "-above"] = b, b + 1
    return out


STEP_CASES = ("one", "bn_small_rows-below", "bn_small_rows-above", "bn_max_gemm_tiles-below", "bn_max_gemm_tiles-above", "bn_chunk_cap-below",
              "bn_chunk_cap-above", "bn_max_chunks-below", "bn_max_chunks-above", "reference-batch")


def _device_signs(tr, B, stem_mask):
    """Per layer, which outputs of the last forward pass came out of their ReLU positive.  The stem's activation has been through its
    dropout in place: where that dropped a cell the side is unknown (and without consequence), None leaves it to the oracle."""
    signs = [(a > 0).cpu().numpy().reshape(B, 25, 20, 64) for a in tr._ws[B]["A"]]
    return signs, stem_mask != 0


def _oracle_step(tr, B, x, y, masks, weight_decay=0.0, named=None):
    """The oracle's step, with the ReLU cells the device cannot tell from zero resolved the way the device resolved them
    (dscnn_train_cases.forward): the reference of everything but those sides stays the float64 oracle.  A plain oracle step tells the
    stem's dropped cells (the device's side is unknown there) -- they keep the oracle's side."""
    named = named if named is not None else cases.tensors64(cases.params())
    signs, kept = _device_signs(tr, B, masks[0])
    signs[0] = np.where(kept, signs[0], _stem_side(named, x))
    want = cases.step(named, x, y, masks, weight_decay, signs=signs)
    cells = B * 25 * 20 * 64
    print(f"ReLU cells within {cases.KINK:g} of zero taken from the device, per layer: {want['kinks']} of {cells}; flipped beyond: {want['flipped']}")
    assert not any(want["flipped"]) and sum(want["kinks"]) <= 1e-5 * 9 * cells + 4, (want["kinks"], want["flipped"])
    return want


def _stem_side(named, x):
    t = {n: torch.from_numpy(np.asarray(v, dtype=np.float64)) for n, v in named.items()}
    z = F.conv2d(F.pad(torch.from_numpy(np.asarray(x, dtype=np.float64))[:, None], (1, 1, 4, 5)), t["conv2d/kernel"].permute(3, 2, 0, 1), stride=2)
    z = z + t["conv2d/bias"].view(1, -1, 1, 1)
    y = cases._bn(z, t, "batch_normalization", True, dict(batch={}, moving={}))
    return (y > 0).permute(0, 2, 3, 1).numpy()


def _assert_grads(got, want, bound=1e-3):
    print("gradient errors / max |reference|: " + ", ".join(f"{n} {_rel(got[n], g):.1e}" for n, g in want.items() if n not in cases.CONV_BIASES))
    for name, g in want.items():
        if name in cases.CONV_BIASES:
            assert not got[name].any(), name
        else:
            assert _rel(got[name], g) <= bound, (name, _rel(got[name], g))


@pytest.mark.parametrize("case", STEP_CASES)
def test_whole_step(ops, case):
    B = _route_batches(ops)[case]
    tr = dscnn_trainer.DSCNNTrainer(cases.params(), max_batch=B, seed=MASK_SEED, weight_decay=0.0)
    x, y = cases.clips(100)[:B], cases.labels_for(B)
    stats = tr.forward_backward(x, y).cpu().tolist()
    want = _oracle_step(tr, B, x, y, cases.host_masks(MASK_SEED, 0, B))
    print(f"{case}: B {B} loss {stats[0] / B:.8f} (oracle {want['loss']:.8f}) correct {stats[1]} ({want['correct']})")
    assert abs(stats[0] / B - want["loss"]) <= 1e-5 * abs(want["loss"]) and int(stats[1]) == want["correct"]
    _assert_grads(tr.named_grads(), want["grads"])
    batch, exported = tr.batch_statistics(), dscnn.unpack(tr.params())
    for prefix, (mean, var) in want["batch"].items():
        assert _rel(batch[prefix][0], mean) <= 1e-5 and _rel(batch[prefix][1], var) <= 1e-5, prefix
    for name, value in want["moving"].items():
        assert _rel(exported[name], value) <= 1e-5, name
    for name, value in dscnn.unpack(cases.params()).items():           # the optimizer has not run: nothing else moved
        if name not in want["moving"]:
            assert np.array_equal(exported[name], value), name


def test_l2(ops):
    B = 3
    grads = []
    for wd in (0.0, 1e-4):
        tr = dscnn_trainer.DSCNNTrainer(cases.params(), max_batch=B, seed=MASK_SEED, weight_decay=wd)
        tr.forward_backward(cases.clips(100)[:B], cases.labels_for(B))
        grads.append(tr.named_grads())
    W = dscnn.unpack(cases.params())
    for name in grads[0]:
        diff = grads[1][name].astype(np.float64) - grads[0][name]
        if name in cases.CONV_KERNELS:
            assert np.abs(diff - 2e-4 * W[name].astype(np.float64)).max() <= 1e-6 * np.abs(W[name]).max(), name
        else:
            assert not diff.any(), name
    want = 1e-4 * sum((W[k].astype(np.float64) ** 2).sum() for k in cases.CONV_KERNELS)
    assert abs(tr.regularization_loss() - want) <= 1e-9 * want
    _assert_grads(grads[1], _oracle_step(tr, B, cases.clips(100)[:B], cases.labels_for(B), cases.host_masks(MASK_SEED, 0, B), 1e-4)["grads"])


def test_adam_step_and_the_step_after(ops):
    B, lr = 3, 5e-4
    x, y = cases.clips(100)[:B], cases.labels_for(B)
    tr = dscnn_trainer.DSCNNTrainer(cases.params(), max_batch=B, seed=MASK_SEED, weight_decay=0.0)
    tr.forward_backward(x, y)
    before, grads = dscnn.unpack(tr.params()), tr.named_grads()
    tr.adam_step(lr)
    assert tr.step_count == 1
    after = dscnn.unpack(tr.params())
    for name, p in before.items():
        if cases.trainable(name) and name not in cases.CONV_BIASES:
            g = grads[name].astype(np.float64)
            want, _, _ = cases.adam(p.astype(np.float64), g, np.zeros_like(g), np.zeros_like(g), 1, lr)
            assert np.abs(after[name] - want).max() <= 1e-6 * np.abs(p).max(), name
            assert not np.array_equal(after[name], p), name
        else:                            # conv biases; moving statistics are not the optimizer's
            assert np.array_equal(after[name], p), name
    # the tape runs on the updated weights, and the masks are those of step 1
    second = cases.tensors64(tr.params())
    stats = tr.forward_backward(x, y).cpu().tolist()
    want = _oracle_step(tr, B, x, y, cases.host_masks(MASK_SEED, 1, B), named=second)
    assert abs(stats[0] / B - want["loss"]) <= 1e-5 * abs(want["loss"])
    _assert_grads(tr.named_grads(), want["grads"])


def _run_steps(mode, n=3, B=3, seed=5):
    tr = dscnn_trainer.DSCNNTrainer(cases.params(), max_batch=8, seed=seed, mode=mode)
    kept = []
    for s in range(n):
        tr.step(cases.clips(100)[s * B:(s + 1) * B], cases.labels_for(B), 5e-4)
        kept.append((tr._ws[B]["A"][0] != 0).cpu().numpy())           # the stem's activation after its dropout
    return tr, kept


def test_determinism_and_hipgraph(ops):
    a, kept_a = _run_steps("eager")
    b, _ = _run_steps("eager")
    c, kept_c = _run_steps("hipgraph")
    assert a.step_count == b.step_count == c.step_count == 3
    for other in (b, c):
        for mine, theirs in ((a.params_dev, other.params_dev), (a.m, other.m), (a.v, other.v), (a.grads, other.grads), (a.stats, other.stats)):
            assert torch.equal(mine, theirs)
    for kept in (kept_a, kept_c):
        # the dropped cells of live activations differ from step to step: a replay draws fresh masks
        assert not np.array_equal(kept[0], kept[1]) and not np.array_equal(kept[1], kept[2])
    # a batch of another size runs eager on the same trainer
    c.step(cases.clips(100)[:2], cases.labels_for(2), 5e-4)
    a.step(cases.clips(100)[:2], cases.labels_for(2), 5e-4)
    assert torch.equal(a.params_dev, c.params_dev) and c.step_count == 4


def test_export(ops):
    tr, _ = _run_steps("eager", n=2)
    blob = tr.params()
    x = cases.clips(100)[:5]
    model = dscnn.DSCNN(blob, max_batch=8)
    want = dscnn.dscnn_host(x, blob)
    assert _rel(model.logits(torch.from_numpy(np.asarray(x)).cuda()).cpu().numpy(), want) <= 1e-5
    model.close()
    assert not np.array_equal(blob, cases.params())


def test_it_learns(ops):
    """The bar is the float64 oracle's (tests/test_dscnn_train_cpu.py asserts the three accuracies it comes from); the device runs the same
    batches under a mask seed of its own."""
    train, (held_x, held_y) = cases.task_batches()
    tr = dscnn_trainer.DSCNNTrainer(cases.task_start(), max_batch=cases.TASK_BATCH, seed=4, weight_decay=1e-4)
    for x, y in train:
        tr.step(x, y, cases.TASK_LR)
    model = dscnn.DSCNN(tr.params(), max_batch=cases.TASK_HELD_OUT)
    accuracy = float((model.predict(held_x).argmax(axis=1) == held_y).mean())
    model.close()
    print(f"held-out accuracy {accuracy:.4f}, bar {cases.TASK_BAR:.4f}")
    assert accuracy >= cases.TASK_BAR


def test_train(ops, tmp_path):
    from multilingual_kws_amd.embedding import input_data
    words, files = ("left", "right"), {"train": [], "val": [], "unknown": []}
    pcm = synth.clips_int16(2 * 7 + 6, seed=0x7123)
    at = 0
    for w in words:
        for i in range(7):                                             # 5 to train on (10 in all: batches of 8 and 2), 2 to validate on
            path = tmp_path / w / f"{w}{i}.wav"
            path.parent.mkdir(exist_ok=True)
            path.write_bytes(synth.wav_bytes(pcm[at]))
            files["train" if i < 5 else "val"].append(str(path))
            at += 1
    for i in range(6):
        path = tmp_path / "other" / f"o{i}.wav"
        path.parent.mkdir(exist_ok=True)
        path.write_bytes(synth.wav_bytes(pcm[at + i]))
        files["unknown"].append(str(path))
    bg = tmp_path / "_background_noise_"
    bg.mkdir()
    (bg / "bg0.wav").write_bytes(synth.wav_bytes(synth.clips_int16(1, num_samples=32000, seed=0xB6)[0] // 8))
    ms = input_data.standard_microspeech_model_settings(4)            # silence, unknown, left, right
    assert len(files["train"]) % 8 != 0
    model = dscnn_comparison.train(list(words), files["train"], files["val"], files["unknown"], ms, "toy", str(bg), epochs=2, batch_size=8,
                                   checkpoint_dir=str(tmp_path / "checkpoints"), verbose=0)
    assert sorted(model.history) == ["loss", "lr", "sparse_categorical_accuracy", "val_loss", "val_sparse_categorical_accuracy"]
    assert all(len(v) == 2 and np.all(np.isfinite(v)) for v in model.history.values()) and model.history["lr"] == [0.0005, 0.0005]
    loaded = dscnn.DSCNN.load(os.path.join(str(tmp_path / "checkpoints"), "dscnn_toy"), max_batch=8)
    assert loaded.label_count == 4
    loaded.close()
    got = dscnn_comparison.evaluate(model, files["val"], [2, 2, 3, 3], ms)
    assert got["confusion_matrix"].sum() == 4 and 0.0 <= got["accuracy"] <= 1.0
    model.close()
