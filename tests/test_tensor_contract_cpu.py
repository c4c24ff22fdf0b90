"""The tensor contract of the core wrappers, host side: every check_* function on CPU tensors.  The well-formed call
returns the sizes the wrapper derives, every accepted variant passes, and every violation of tests/util_tensor_contract.py -- each one change
to one argument -- raises ValueError (TypeError where the wrapper always raised that) in a message that names the argument.  The wrong
device is torch.device("meta") against an expected CPU device, as in tests/test_live_routes_cpu.py.  No GPU."""
import re
import types

import pytest

torch = pytest.importorskip("torch")

from tests import util_tensor_contract as tc  # noqa: E402

CPU = torch.device("cpu")
ENTRIES = tc.cpu_entries()


def _surroundings():
    return tc.surroundings("cpu", "meta", other=tc._head_like(tc.OTHER_DIMS), closed=tc._head_like(h=None), far=tc._head_like(dev="meta"))


def _fill(entry):
    return dict(heads=[tc._head_like() for _ in range(3)]) if entry is tc.HEAD_FORWARD_MANY else {}


@pytest.mark.parametrize("entry", ENTRIES, ids=lambda e: e["name"])
def test_well_formed_arguments_give_the_sizes_the_wrapper_derives(entry):
    assert tc.call_check(entry, tc.arguments(entry, CPU, **_fill(entry)), CPU) == entry["returns"]


@pytest.mark.parametrize("entry", ENTRIES, ids=lambda e: e["name"])
def test_accepted_variants_pass(entry):
    x = _surroundings()
    for case in entry["accepted"]:
        tc.call_check(entry, tc.changed(entry, case, x, **_fill(entry)), CPU)          # (raises if refused)


@pytest.mark.parametrize("entry", ENTRIES, ids=lambda e: e["name"])
def test_every_violation_is_refused_in_a_message_that_names_the_argument(entry):
    x = _surroundings()
    assert entry["violations"]
    for case in entry["violations"]:
        label, names = case[0], case[1]
        a = tc.changed(entry, case, x, **_fill(entry))
        with pytest.raises(tc.exception_of(case)) as ei:
            tc.call_check(entry, a, CPU)
        assert isinstance(ei.value, ValueError) == (tc.exception_of(case) is ValueError), label
        word = "audio" if tc.exception_of(case) is TypeError else names          # (Frontend.forward's TypeError, kept as it was: "audio must be float32 or int16")
        assert re.search(rf"\b{word}\b", str(ei.value)), (label, str(ei.value))


@pytest.mark.parametrize("entry", [e for e in ENTRIES if not e.get("partial")], ids=lambda e: e["name"])
def test_the_tables_cover_every_tensor_argument_of_the_check(entry):
    """The keys of the violation table against the check function's signature: an argument added to a wrapper's check without cases fails here."""
    covered = {n for case in entry["violations"] for n in (case[1] if isinstance(case[1], tuple) else (case[1],))}
    assert covered == tc.tensor_parameters(entry), entry["name"]
    kinds = {}
    for case in entry["violations"]:
        kinds.setdefault(case[1], []).append(case[0])
    for name, labels in kinds.items():
        if name in ("heads", "spec") or entry is tc.KMEANS_NEAREST_OUT:
            continue
        text = " | ".join(labels)
        assert "another device" in text, (entry["name"], name)                   # every tensor: a wrong device
        assert re.search(r"float|int|bool", text), (entry["name"], name)          # ... and a wrong dtype


def test_every_mandatory_entry_point_has_an_entry():
    names = {e["name"].split("[")[0] for e in ENTRIES}
    assert names >= {"Head.forward", "Head.forward_many", "Head.loss_grad", "Head.adam_step_dev", "EmbeddingModel.forward", "Frontend.forward",
                     "Frontend.stream", "Frontend.live_push", "detector.detect_live_step", "kmeans.nearest_on_device(out=)"}


def test_the_checks_touch_no_tensor_data():
    """Meta tensors have no storage: a check that copied, compared or allocated from its arguments would fail on them.  With everything on
    the meta device and that as the expected device, every well-formed call passes."""
    meta = torch.device("meta")
    for entry in ENTRIES:
        a = tc.arguments(entry, "cpu", **_fill(entry))
        a = {k: (v.to(meta) if torch.is_tensor(v) else tuple(t.to(meta) for t in v) if isinstance(v, tuple) else v) for k, v in a.items()}
        if entry is tc.HEAD_FORWARD_MANY:
            a["heads"] = [tc._head_like(dev="meta") for _ in range(3)]
        assert tc.call_check(entry, a, meta) == entry["returns"], entry["name"]


def test_a_state_size_the_library_has_no_answer_for_is_left_to_the_c_call():
    """mkws_detect_live_state_bytes gives 0 for arguments the C call refuses in its own words (a history above the cap): the wrapper's check
    does not judge the state then, so that the caller sees the library's error (tests/test_live_detector_gpu.py pins its code)."""
    from multilingual_kws_amd import detector, frontend
    entry = tc.live_step_entry(1)
    a = tc.arguments(entry, CPU)
    assert detector.check_live_step(CPU, history=detector.LIVE_MAX_HISTORY + 1, **a) == entry["returns"]
    push = tc.live_push_entry(1)
    a = tc.arguments(push, CPU)
    assert frontend.check_live_push(frontend.make_cfg(), CPU, 0, window_samples=tc.CLIP, hop_samples=tc.HOP, hops_per_push=1, **a) == 49


def test_many_stream_tensors_of_another_dtype_or_device_are_named():
    from multilingual_kws_amd.frontend import check_live_many_tensors
    good = dict(states=(torch.zeros((2, 4), dtype=torch.int64), torch.int64), active=(None, torch.int32), out=(torch.zeros(3), torch.float32))
    check_live_many_tensors("f", CPU, **good)
    for name, t in (("states", torch.zeros((2, 4), dtype=torch.int64, device="meta")), ("states", torch.zeros((2, 4), dtype=torch.int32)),
                    ("active", torch.zeros(2, dtype=torch.int64)), ("out", torch.zeros(3, device="meta")), ("out", torch.zeros(3, dtype=torch.float64))):
        with pytest.raises(ValueError, match=rf"\b{name}\b"):
            check_live_many_tensors("f", CPU, **dict(good, **{name: (t, good[name][1])}))


def test_trainer_checks():
    from multilingual_kws_amd import embedding_trainer as et
    spec = torch.zeros((4, 49, 40))
    assert et.check_forward_train(CPU, spec) == 4 and et.check_forward_train(CPU, torch.zeros((2, 49, 40, 1), dtype=torch.float64)) == 2
    for bad in (torch.zeros((4, 49, 41)), torch.zeros((4, 48, 40)), torch.zeros((49, 40)), torch.zeros((4, 49, 40, 2)), [[0.0] * 40] * 49):
        with pytest.raises(ValueError, match=r"\bspec\b"):
            et.check_forward_train(CPU, bad)
    # the per-block scales are read by the residual kernels as they are (B floats); the masks are converted and uploaded by the wrapper
    scales = {"2b": torch.ones(4), "3b": torch.ones(8)[::2]}
    masks = {"2b": [True, False, True, True], "3b": torch.ones(4, dtype=torch.bool), "4b": __import__("numpy").ones(4, bool)}
    assert et.check_forward_train(CPU, spec, masks, scales) == 4 and et.check_forward_train(CPU, spec, None, {}) == 4
    meta = torch.device("meta")
    assert et.check_forward_train(meta, spec.to(meta), None, {k: v.to(meta) for k, v in scales.items()}) == 4
    for bad in (torch.ones(4, dtype=torch.float64), torch.ones(4, dtype=torch.float16), torch.ones(4, dtype=torch.int32), torch.ones(3), torch.ones(5),
                torch.ones((4, 1)), torch.ones(4, device="meta"), [1.0] * 4):
        with pytest.raises(ValueError, match=r"\bkeep_scales\['3b'\]"):
            et.check_forward_train(CPU, spec, None, dict(scales, **{"3b": bad}))
    for bad in ([True] * 3, [True] * 5, torch.ones((4, 1), dtype=torch.bool), True):
        with pytest.raises(ValueError, match=r"\bdrop_masks\['3b'\]"):
            et.check_forward_train(CPU, spec, dict(masks, **{"3b": bad}))
    et.check_backward(4, torch.zeros((4, 1024)))
    for bad in (torch.zeros((3, 1024)), torch.zeros((5, 1024)), torch.zeros((4, 1023)), torch.zeros(4 * 1024), None):
        with pytest.raises(ValueError, match=r"\bd_emb\b"):
            et.check_backward(4, bad)


def test_indexed_device():
    from multilingual_kws_amd import _lib
    assert _lib.indexed_device("cpu") == CPU and _lib.indexed_device(torch.device("cuda:3")) == torch.device("cuda", 3)
    assert _lib.indexed_device("cuda:0").index == 0


def test_the_proxy_forwards_host_queries_only():
    real = types.SimpleNamespace(mkws_last_error=lambda: b"", mkws_head_forward=lambda *a: 0)
    proxy = tc.HostOnlyLibrary(real)
    assert proxy.mkws_last_error() == b"" and proxy.queries == ["mkws_last_error"]
    with pytest.raises(AssertionError):
        proxy.mkws_head_forward
    assert proxy.refused == ["mkws_head_forward"]
    # every allow-listed name is a symbol the library exports (that none takes a device pointer or a stream is read off include/mkws.h)
    symbols = {name: args for name, _, args in tc._lib.SYMBOLS}
    assert tc.HOST_QUERIES <= set(symbols)
