"""The float64 oracle of the DS-CNN training step (tests/dscnn_train_cases.py) and the host logic of dscnn_trainer / dscnn_comparison,
without a GPU: the oracle is checked against the inference specification, against finite differences and for being a usable test input
before tests/test_dscnn_train_gpu.py holds the device to it."""
import numpy as np
import pytest

from multilingual_kws_amd import dscnn, dscnn_comparison, dscnn_trainer
from tests import dscnn_train_cases as cases

B = 6


@pytest.fixture(scope="module")
def one_step():
    named = cases.tensors64(cases.params())
    return named, cases.step(named, cases.clips(B), cases.labels_for(B), cases.host_masks(11, 0, B), weight_decay=1e-4)


def test_eval_mode_is_the_inference_specification():
    """Unfolded float64 against dscnn_host, which goes through float32 folded weights: 1e-6 of max |value|."""
    want = dscnn.dscnn_host(cases.clips(B), cases.params())
    got = cases.eval_logits(cases.tensors64(cases.params()), cases.clips(B))
    assert np.abs(got - want).max() <= 1e-6 * np.abs(want).max()


def test_finite_differences(one_step):
    named, r = one_step
    x, y, masks = cases.clips(B), cases.labels_for(B), cases.host_masks(11, 0, B)
    rng = np.random.default_rng(0)
    gmax = max(np.abs(r["grads"][k]).max() for k in cases.CONV_KERNELS)
    for name, g in r["grads"].items():
        for _ in range(3):
            idx = tuple(int(rng.integers(0, d)) for d in g.shape)
            h = 1e-7 * max(1.0, abs(named[name][idx]))       # (small: every step crosses ReLU kinks in proportion to h)
            up, down = {**named, name: named[name].copy()}, {**named, name: named[name].copy()}
            up[name][idx] += h
            down[name][idx] -= h
            fd = (cases.loss_only(up, x, y, masks, 1e-4) - cases.loss_only(down, x, y, masks, 1e-4)) / (2 * h)
            assert abs(fd - g[idx]) <= 1e-6 * gmax + 1e-5 * abs(g[idx]), (name, idx, fd, g[idx])


def test_conv_bias_gradients_vanish(one_step):
    """Under batch statistics the batch mean removes a bias in front of a BatchNorm: what is left is rounding noise.  This is why the
    device defines these nine gradients as zero."""
    _, r = one_step
    gmax = max(np.abs(r["grads"][k]).max() for k in cases.CONV_KERNELS)
    for bias in cases.CONV_BIASES:
        assert np.abs(r["grads"][bias]).max() < 1e-9 * gmax, bias


def test_every_other_gradient_is_non_zero(one_step):
    _, r = one_step
    for name, g in r["grads"].items():
        if name not in cases.CONV_BIASES:
            assert np.abs(g).max() > 0 and np.all(np.isfinite(g)), name
    assert len(set(cases.labels_for(B).tolist())) >= 3


def test_relus_alive_under_batch_statistics():
    alive = []
    cases.forward(cases.tensors64(cases.params()), cases.clips(B), None, training=True, alive=alive)
    assert len(alive) == 9 and all(0.2 <= a <= 0.8 for a in alive), alive


def test_dropout_mask_host():
    n, rate = 32000, 0.4
    a = dscnn_trainer.dropout_mask_host(5, 3, 1, n, rate)
    assert a.dtype == np.bool_ and np.array_equal(a, dscnn_trainer.dropout_mask_host(5, 3, 1, n, rate))
    assert not np.array_equal(a, dscnn_trainer.dropout_mask_host(5, 4, 1, n, rate))
    assert not np.array_equal(a, dscnn_trainer.dropout_mask_host(5, 3, 0, n, rate))
    assert not np.array_equal(a, dscnn_trainer.dropout_mask_host(6, 3, 1, n, rate))
    for r in (0.2, 0.4):
        share = dscnn_trainer.dropout_mask_host(9, 0, 0, n, r).mean()
        assert abs(share - (1 - r)) <= 4 * np.sqrt(r * (1 - r) / n), (r, share)
    assert dscnn_trainer.dropout_mask_host(1, 0, 0, 1000, 0.0).all()
    # a prefix of a longer mask: the decision of element i depends on i alone
    assert np.array_equal(a[:100], dscnn_trainer.dropout_mask_host(5, 3, 1, 100, rate))


def test_step_function_is_the_references():
    f = dscnn_comparison.step_function_wrapper(100)
    assert [f(e, 123.0) for e in (0, 11, 12, 23, 24, 35, 36, 47)] == [0.0005, 0.0005, 0.0001, 0.0001, 0.00002, 0.00002, 0.00001, 0.00001]


def test_the_oracle_learns_the_task():
    """The bar of test_dscnn_train_gpu.py::test_it_learns comes from here: three mask seeds, the accuracies recorded in the cases."""
    got = tuple(cases.oracle_train(seed) for seed in cases.TASK_MASK_SEEDS)
    assert got == cases.TASK_ORACLE_ACCURACY, got
    assert cases.TASK_BAR > 1.0 / cases.TASK_CLASSES + 0.4       # far above chance: the device test means something
