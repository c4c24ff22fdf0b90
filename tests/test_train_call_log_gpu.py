"""-m gpu: the library calls one optimizer step of every trainer over the mkws_op_* operators makes, against tests/golden/train_call_log.json
(recorded by tests/golden/make_train_call_log.py at commit e976235, before the trainers moved onto op_tape.OpTape): EmbeddingTrainer with the
default switches, four switch variants and the keep-scales form, DSCNNTrainer with and without weight decay, LogitsLayer.  The host code above
the operators may be rearranged; the sequence of calls and their arguments (normalised as the generator's docstring says) may not."""
import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu
pytest.importorskip("torch")

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def gen():
    spec = importlib.util.spec_from_file_location("make_train_call_log", os.path.join(HERE, "golden", "make_train_call_log.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def logs(gen):
    return gen.record_all()


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(HERE, "golden", "train_call_log.json")) as f:
        return json.load(f)


def test_the_golden_file_holds_every_case(gen, logs, golden):
    assert set(golden["calls"]) == set(gen.FULL) and set(golden["calls"]) | set(golden["sha256"]) == set(logs)
    assert len(golden["sha256"]) == 6 and all(len(log) > 0 for log in logs.values())


@pytest.mark.parametrize("case", ["embedding", "dscnn", "logits"])
def test_default_case_makes_the_recorded_calls(logs, golden, case):
    got, want = logs[case], golden["calls"][case]
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, f"{case}: call {i} differs: got {g}, recorded {w}"
    assert len(got) == len(want), f"{case}: {len(got)} calls, recorded {len(want)}; first unmatched: {max(got, want, key=len)[min(len(got), len(want))]}"


@pytest.mark.parametrize("case", ["embedding/no_wgrad_stream", "embedding/fuse_bn_stats_0", "embedding/fuse_bn_stats_7", "embedding/wgrad_fork_every_2",
                                  "embedding/keep_scales", "dscnn/no_weight_decay"])
def test_variant_case_makes_the_recorded_calls(gen, logs, golden, case):
    assert gen.digest(logs[case]) == golden["sha256"][case], f"{case}: {len(logs[case])} calls hash differently from the recorded log"
