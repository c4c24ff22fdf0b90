"""The tensor contract of the core wrappers as case tables, shared by tests/test_tensor_contract_cpu.py (the pure
check_* functions on CPU tensors) and tests/test_tensor_contract_gpu.py (the wrappers themselves, behind a library proxy).

An ENTRY describes one entry point: the check function, its plain arguments, a builder of the well-formed tensor arguments, the sizes the
check returns for them, the accepted variants and the violations.  A violation or variant is (label, argument, change[, exception]):
`change(a, x)` returns the new value of that ONE argument; `a` is a fresh copy of the well-formed arguments, `x` the surroundings -- x.dev
(the device everything lives on), x.bad_dev (a device a tensor must not be on: "meta" against an expected CPU device, the CPU against a
CUDA one) and, for Head.forward_many, x.other / x.closed / x.far (a head of other dimensions, a closed one, one on another device).

No test here ever hands a refused tensor to the device: the GPU file runs every violation with the library replaced by HostOnlyLibrary."""
import inspect
import types

import numpy as np
import torch

from multilingual_kws_amd import _lib, detector, embedding_model, frontend, head, kmeans

# The pure host queries a wrapper may make before it has accepted its arguments: functions of include/mkws.h whose C signature has neither
# a device pointer nor a stream.  Everything else reaches (or may reach) the device and fails the test.
HOST_QUERIES = frozenset([
    "mkws_last_error", "mkws_abi_version", "mkws_build_arch",
    "mkws_frontend_num_frames", "mkws_frontend_live_state_bytes", "mkws_frontend_default_cfg",
    "mkws_detect_live_state_bytes",
    "mkws_head_param_count", "mkws_head_grad_count", "mkws_head_state_floats", "mkws_dscnn_param_count",
    "mkws_resample_geometry", "mkws_resample_out_samples", "mkws_resample_live_in_samples", "mkws_resample_live_state_bytes",
])


class HostOnlyLibrary:
    """Stands in for the ctypes library: forwards HOST_QUERIES, records and refuses everything else."""

    def __init__(self, real):
        self._real, self.queries, self.refused = real, [], []

    def __getattr__(self, name):
        if name in HOST_QUERIES:
            self.queries.append(name)
            return getattr(self._real, name)
        self.refused.append(name)
        raise AssertionError(f"{name} was called: a refusal must be decided before any device call")


def surroundings(dev, bad_dev, **more):
    return types.SimpleNamespace(dev=torch.device(dev), bad_dev=torch.device(bad_dev), **more)


def rand(shape, dev, seed=0, dtype=torch.float32):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(shape, generator=g) * 2 - 1).to(dtype).to(dev)


def zeros(shape, dtype, dev):
    return torch.zeros(shape, dtype=dtype, device=dev)


# ---- generic changes -------------------------------------------------------------------------------------------------------------------

def as_dtype(name, dtype):
    return lambda a, x: a[name].to(dtype)


def on_bad_device(name):
    return lambda a, x: torch.zeros(a[name].shape, dtype=a[name].dtype, device=x.bad_dev)


def reshaped(name, *shape):
    return lambda a, x: a[name].reshape(*shape)


def fewer_rows(name, k=1):
    return lambda a, x: a[name][:a[name].shape[0] - k].contiguous()


def short_by_one(name):
    """The same storage kind, one element short (flat)."""
    return lambda a, x: a[name].reshape(-1)[:-1]


def every_other(name, dim=-1):
    """A view with stride 2 along `dim` of a buffer twice as wide: the right shape and dtype, not contiguous."""
    def change(a, x):
        t = a[name]
        shape = list(t.shape)
        d = dim % t.dim()
        shape[d] *= 2
        wide = torch.zeros(shape, dtype=t.dtype, device=t.device)
        return wide[(slice(None),) * d + (slice(None, None, 2),)]
    return change


def column_slice(name, extra=7):
    """A [:, ..., :w] view of a buffer `extra` columns wider: the right shape and dtype, rows not back to back."""
    def change(a, x):
        t = a[name]
        wide = torch.zeros(tuple(t.shape[:-1]) + (t.shape[-1] + extra,), dtype=t.dtype, device=t.device)
        wide[..., :t.shape[-1]] = t
        return wide[..., :t.shape[-1]]
    return change


def transposed(name):
    return lambda a, x: torch.zeros(tuple(reversed(a[name].shape)), dtype=a[name].dtype, device=a[name].device).permute(*reversed(range(a[name].dim())))


def off_by_one_element(name):
    """The same values in storage that starts one element after a 256-byte boundary (4-byte alignment for float32, 2-byte for int16)."""
    def change(a, x):
        t = a[name]
        base = torch.zeros(t.numel() + 1, dtype=t.dtype, device=t.device)
        view = base[1:].view(t.shape)
        view.copy_(t)
        return view
    return change


def float_dtypes(name):
    """float64, float16 and int32 where float32 is wanted."""
    return [(f"{name} float64", name, as_dtype(name, torch.float64)), (f"{name} float16", name, as_dtype(name, torch.float16)),
            (f"{name} int32", name, as_dtype(name, torch.int32))]


# ---- the entry points ------------------------------------------------------------------------------------------------------------------

IN, HID, CLS, B_HEAD = 1024, 18, 3, 5                 # the head of the product; the second head of forward_many's refusals is 64 x 4 x 2
OTHER_DIMS = (64, 4, 2)


def _emb_violations(B_matters=False):
    v = float_dtypes("emb") + [("emb on another device", "emb", on_bad_device("emb")), ("emb of rank 1", "emb", lambda a, x: a["emb"][0]),
                               ("emb of rank 3", "emb", lambda a, x: a["emb"][:, :, None]), ("emb of width 512", "emb", lambda a, x: a["emb"][:, :512]),
                               ("emb of width in + 1", "emb", lambda a, x: torch.cat([a["emb"], a["emb"][:, :1]], dim=1))]
    if B_matters:
        v.append(("emb one row short of labels", "emb", fewer_rows("emb")))
    return v


_EMB_ACCEPTED = [("emb as a column slice of a wider buffer", "emb", column_slice("emb")),
                 ("emb one float past a 256-byte boundary", "emb", off_by_one_element("emb"))]


def _head_like(dims=(IN, HID, CLS), dev="cpu", h=1):
    return types.SimpleNamespace(in_dim=dims[0], hidden=dims[1], classes=dims[2], device=torch.device(dev), h=h)


HEAD_FORWARD = dict(
    name="Head.forward", check=head.check_forward, plain=dict(in_dim=IN), returns=B_HEAD,
    tensors=lambda dev: dict(emb=rand((B_HEAD, IN), dev, 1)),
    accepted=_EMB_ACCEPTED, violations=_emb_violations())

HEAD_FORWARD_MANY = dict(
    name="Head.forward_many", check=head.check_forward_many, plain=dict(), returns=(3, B_HEAD), no_device=True,
    tensors=lambda dev: dict(heads=None, emb=rand((B_HEAD, IN), dev, 1)),          # heads: filled in by the test (stand-ins on the CPU, Heads on the GPU)
    accepted=_EMB_ACCEPTED + [("one head", "heads", lambda a, x: a["heads"][:1]), ("a head twice", "heads", lambda a, x: a["heads"][:1] * 2)],
    violations=_emb_violations() + [
        ("heads empty", "heads", lambda a, x: []), ("heads of unequal dimensions", "heads", lambda a, x: a["heads"][:2] + [x.other]),
        ("heads: the first one differs", "heads", lambda a, x: [x.other] + a["heads"]), ("heads with a closed one", "heads", lambda a, x: a["heads"][:1] + [x.closed]),
        ("heads on different devices", "heads", lambda a, x: a["heads"][:1] + [x.far])])

HEAD_LOSS_GRAD = dict(
    name="Head.loss_grad", check=head.check_loss_grad, plain=dict(in_dim=IN), returns=B_HEAD,
    tensors=lambda dev: dict(emb=rand((B_HEAD, IN), dev, 1), labels=torch.tensor([0, 1, 2, 2, 1], dtype=torch.int32, device=dev)),
    accepted=_EMB_ACCEPTED + [("labels int64", "labels", as_dtype("labels", torch.int64)), ("labels uint8", "labels", as_dtype("labels", torch.uint8)),
                              ("labels strided", "labels", lambda a, x: torch.stack([a["labels"], a["labels"]], dim=1)[:, 0])],
    violations=_emb_violations(B_matters=True) + [
        ("labels float32", "labels", as_dtype("labels", torch.float32)), ("labels float64", "labels", as_dtype("labels", torch.float64)),
        ("labels bool", "labels", as_dtype("labels", torch.bool)), ("labels on another device", "labels", on_bad_device("labels")),
        ("labels of rank 2", "labels", lambda a, x: a["labels"][:, None]), ("labels one short", "labels", fewer_rows("labels")),
        ("labels one too many", "labels", lambda a, x: torch.cat([a["labels"], a["labels"][:1]]))])

HEAD_ADAM_STEP_DEV = dict(
    name="Head.adam_step_dev", check=head.check_adam_step_dev, plain=dict(), returns=None,
    tensors=lambda dev: dict(d_step=torch.ones(1, dtype=torch.int32, device=dev)),
    accepted=[("d_step as a 0-d tensor", "d_step", lambda a, x: a["d_step"][0]), ("d_step as an element of a longer tensor", "d_step", lambda a, x: torch.ones(4, dtype=torch.int32, device=x.dev)[2:3])],
    violations=[("d_step int64", "d_step", as_dtype("d_step", torch.int64)), ("d_step float32", "d_step", as_dtype("d_step", torch.float32)),
                ("d_step on another device", "d_step", on_bad_device("d_step")), ("d_step of two elements", "d_step", lambda a, x: torch.ones(2, dtype=torch.int32, device=x.dev)),
                ("d_step empty", "d_step", lambda a, x: a["d_step"][:0])])

OUT_DIM, B_EMB = 1024, 3


def embed_entry(output_dim=OUT_DIM, B=B_EMB):
    return dict(
        name=f"EmbeddingModel.forward[{output_dim}]", check=embedding_model.check_forward, plain=dict(output_dim=output_dim), returns=B,
        tensors=lambda dev: dict(spec=rand((B, 49, 40), dev, 2) * 300 + 330, out=zeros((B, output_dim), torch.float32, dev)),
        accepted=[("spec [B,49,40,1]", "spec", lambda a, x: a["spec"][..., None]),
                  ("spec as a view of [B,50,41]", "spec", lambda a, x: torch.cat([torch.cat([a["spec"], a["spec"][:, :1]], 1), torch.zeros((B, 50, 1), device=x.dev)], 2)[:, :49, :40]),
                  ("spec as a float64 NumPy array", "spec", lambda a, x: a["spec"].cpu().numpy().astype(np.float64)),
                  ("spec one float past a 256-byte boundary", "spec", off_by_one_element("spec")),
                  ("no out", "out", lambda a, x: None), ("out with rows to spare", "out", lambda a, x: zeros((B + 2, output_dim), torch.float32, x.dev))],
        violations=[("spec of 41 channels", "spec", lambda a, x: torch.cat([a["spec"], a["spec"][:, :, :1]], 2)), ("spec of 48 frames", "spec", lambda a, x: a["spec"][:, :48]),
                    ("spec of rank 2", "spec", lambda a, x: a["spec"][0]), ("spec [B,49,40,2]", "spec", lambda a, x: torch.stack([a["spec"]] * 2, -1))] +
        float_dtypes("out") + [("out on another device", "out", on_bad_device("out")), ("out flat", "out", reshaped("out", -1)), ("out of rank 3", "out", lambda a, x: a["out"][:, :, None]),
                               ("out one column narrow", "out", lambda a, x: zeros((B, output_dim - 1), torch.float32, x.dev)),
                               ("out a column slice of a wider buffer", "out", column_slice("out")), ("out transposed", "out", transposed("out")),
                               ("out every other row", "out", every_other("out", 0)), ("out one row short", "out", fewer_rows("out"))])


EMBED_FORWARD = embed_entry()

B_FE, CLIP, HOP = 3, 16000, 320


def _fe_plain():
    return dict(cfg=frontend.make_cfg())


FRONTEND_FORWARD = dict(
    name="Frontend.forward", check=frontend.check_forward, plain=_fe_plain, returns=(B_FE, CLIP, 49),
    tensors=lambda dev: dict(audio=rand((B_FE, CLIP), dev, 3) * 0.5, out=zeros((B_FE, 49, 40), torch.float32, dev)),
    accepted=[("audio as a row-strided view", "audio", column_slice("audio", 100)), ("audio int16", "audio", lambda a, x: (a["audio"] * 32768).to(torch.int16)),
              ("audio one float past a 256-byte boundary", "audio", off_by_one_element("audio")),
              ("int16 audio one sample past a 256-byte boundary", "audio", lambda a, x: off_by_one_element("audio")(dict(audio=(a["audio"] * 32768).to(torch.int16)), x)),
              ("no out", "out", lambda a, x: None), ("out with rows to spare", "out", lambda a, x: zeros((B_FE + 1, 49, 40), torch.float32, x.dev))],
    violations=[("audio float64", "audio", as_dtype("audio", torch.float64), TypeError), ("audio float16", "audio", as_dtype("audio", torch.float16), TypeError),
                ("audio int32", "audio", as_dtype("audio", torch.int32), TypeError), ("audio on another device", "audio", on_bad_device("audio")),
                ("audio of rank 3", "audio", lambda a, x: a["audio"][None]), ("audio of rank 0", "audio", lambda a, x: a["audio"][0, 0])] +
    float_dtypes("out") + [("out on another device", "out", on_bad_device("out")), ("out flat", "out", reshaped("out", -1)), ("out of 41 channels", "out", lambda a, x: zeros((B_FE, 49, 41), torch.float32, x.dev)),
                           ("out of 48 frames", "out", lambda a, x: zeros((B_FE, 48, 40), torch.float32, x.dev)), ("out a column slice of a wider buffer", "out", column_slice("out")),
                           ("out transposed", "out", lambda a, x: zeros((B_FE, 40, 49), torch.float32, x.dev).permute(0, 2, 1)), ("out one row short", "out", fewer_rows("out"))])

FRONTEND_FORWARD_1D = dict(                         # the [n] form: one clip, out [1, frames, channels]
    name="Frontend.forward[1-D]", check=frontend.check_forward, plain=_fe_plain, returns=(1, CLIP, 49),
    tensors=lambda dev: dict(audio=rand((CLIP,), dev, 3) * 0.5, out=zeros((1, 49, 40), torch.float32, dev)),
    accepted=[], violations=[("out without its row", "out", lambda a, x: a["out"][:0])], partial=True)

N_STREAM = CLIP + 2 * HOP

FRONTEND_STREAM = dict(
    name="Frontend.stream", check=frontend.check_stream, plain=_fe_plain, returns=(N_STREAM, 49, 3), ints=dict(window_samples=CLIP, hop_samples=HOP),
    tensors=lambda dev: dict(audio=rand((N_STREAM,), dev, 4) * 0.5),
    accepted=[("audio strided", "audio", lambda a, x: torch.stack([a["audio"], a["audio"]], 1)[:, 0]), ("audio one float past a 256-byte boundary", "audio", off_by_one_element("audio"))],
    violations=[("audio int16", "audio", lambda a, x: (a["audio"] * 32768).to(torch.int16)), ("audio float64", "audio", as_dtype("audio", torch.float64)),
                ("audio float16", "audio", as_dtype("audio", torch.float16)), ("audio on another device", "audio", on_bad_device("audio")),
                ("audio [1, n]", "audio", lambda a, x: a["audio"][None]), ("audio of rank 0", "audio", lambda a, x: a["audio"][0])])

STATE_BYTES_CPU = 8 * 1234            # the CPU file has no handle to ask; the GPU file takes mkws_frontend_live_state_bytes of its own


def live_push_entry(h, state_bytes=STATE_BYTES_CPU):
    words = (state_bytes + 7) // 8
    return dict(
        name=f"Frontend.live_push[{h} hops]", check=frontend.check_live_push, plain=lambda: dict(cfg=frontend.make_cfg(), state_bytes=state_bytes), returns=49,
        ints=dict(window_samples=CLIP, hop_samples=HOP, hops_per_push=h),
        tensors=lambda dev: dict(state=zeros(words, torch.int64, dev), audio=rand((h * HOP,), dev, 5) * 0.5, spec=zeros((h, 49, 40), torch.float32, dev),
                                 raw=zeros((h, 49, 40), torch.int16, dev), meta=zeros(2 + h, torch.int64, dev)),
        accepted=[("no spec, raw, meta", ("spec", "raw", "meta"), lambda a, x: None), ("a state block with words to spare", "state", lambda a, x: zeros(words + 3, torch.int64, x.dev)),
                  ("audio one float past a 256-byte boundary", "audio", off_by_one_element("audio"))],
        violations=[("state int32", "state", lambda a, x: zeros(2 * words, torch.int32, x.dev)), ("state float64", "state", as_dtype("state", torch.float64)),
                    ("state on another device", "state", on_bad_device("state")), ("state every other word", "state", every_other("state")),
                    ("state one word short", "state", short_by_one("state")),
                    ("audio int16", "audio", as_dtype("audio", torch.int16)), ("audio float64", "audio", as_dtype("audio", torch.float64)),
                    ("audio on another device", "audio", on_bad_device("audio")), ("audio one sample short", "audio", short_by_one("audio")),
                    ("audio one sample long", "audio", lambda a, x: torch.cat([a["audio"], a["audio"][:1]])), ("audio strided", "audio", every_other("audio"))] +
        float_dtypes("spec") + [("spec on another device", "spec", on_bad_device("spec")), ("spec one element short", "spec", short_by_one("spec")),
                                ("spec a column slice of a wider buffer", "spec", column_slice("spec")), ("spec transposed", "spec", transposed("spec")),
                                ("raw int32", "raw", as_dtype("raw", torch.int32)), ("raw float32", "raw", as_dtype("raw", torch.float32)), ("raw uint8", "raw", as_dtype("raw", torch.uint8)),
                                ("raw on another device", "raw", on_bad_device("raw")), ("raw one element short", "raw", short_by_one("raw")), ("raw a column slice", "raw", column_slice("raw")),
                                ("meta int32", "meta", as_dtype("meta", torch.int32)), ("meta float32", "meta", as_dtype("meta", torch.float32)), ("meta float64", "meta", as_dtype("meta", torch.float64)),
                                ("meta on another device", "meta", on_bad_device("meta")), ("meta one element short", "meta", short_by_one("meta")), ("meta strided", "meta", every_other("meta"))])


N_DET, T_DET, C_DET = 2, 3, 3
HISTORY = detector.live_history(100, HOP)          # the history for a 100 ms average


def live_step_entry(h):
    words = _lib.lib().mkws_detect_live_state_bytes(N_DET, T_DET, HISTORY) // 8
    smaller = _lib.lib().mkws_detect_live_state_bytes(N_DET, T_DET - 1, HISTORY - 1) // 8
    assert 0 < smaller < words
    return dict(
        name=f"detector.detect_live_step[{h} new]", check=detector.check_live_step, plain=dict(history=HISTORY), returns=(N_DET, h, C_DET, T_DET),
        tensors=lambda dev: dict(state=zeros(words, torch.int64, dev), probs=torch.softmax(rand((N_DET, h, C_DET), dev, 6) * 3, -1),
                                 meta=torch.tensor([h, 0] + [20 * i for i in range(h)], dtype=torch.int64, device=dev),
                                 d_thresholds=torch.tensor([0.3, 0.5, 0.7], dtype=torch.float64, device=dev),
                                 out=zeros(detector.live_out_words(N_DET, T_DET, h), torch.int64, dev), scores=zeros((N_DET, h), torch.float64, dev)),
        accepted=[("no out, scores", ("out", "scores"), lambda a, x: None), ("a state block with words to spare", "state", lambda a, x: zeros(words + 5, torch.int64, x.dev)),
                  ("meta with elements to spare", "meta", lambda a, x: torch.cat([a["meta"], a["meta"][:3]]))],
        violations=[("state int32", "state", lambda a, x: zeros(2 * words, torch.int32, x.dev)), ("state float64", "state", as_dtype("state", torch.float64)),
                    ("state on another device", "state", on_bad_device("state")), ("state every other word", "state", every_other("state")),
                    ("state one word short", "state", short_by_one("state")),
                    ("state made for fewer thresholds and a shorter history", "state", lambda a, x: zeros(smaller, torch.int64, x.dev))] +
        float_dtypes("probs") + [("probs on another device", "probs", on_bad_device("probs")), ("probs of rank 2", "probs", lambda a, x: a["probs"][0]),
                                 ("probs every other class", "probs", every_other("probs")),
                                 ("meta int32", "meta", as_dtype("meta", torch.int32)), ("meta float32", "meta", as_dtype("meta", torch.float32)),
                                 ("meta on another device", "meta", on_bad_device("meta")), ("meta one element short", "meta", short_by_one("meta")), ("meta strided", "meta", every_other("meta")),
                                 ("d_thresholds float32", "d_thresholds", as_dtype("d_thresholds", torch.float32)), ("d_thresholds int64", "d_thresholds", as_dtype("d_thresholds", torch.int64)),
                                 ("d_thresholds on another device", "d_thresholds", on_bad_device("d_thresholds")), ("d_thresholds strided", "d_thresholds", every_other("d_thresholds")),
                                 ("out int32", "out", as_dtype("out", torch.int32)), ("out float64", "out", as_dtype("out", torch.float64)), ("out on another device", "out", on_bad_device("out")),
                                 ("out one word short", "out", short_by_one("out")), ("out every other word", "out", every_other("out")),
                                 ("scores float32", "scores", as_dtype("scores", torch.float32)), ("scores int64", "scores", as_dtype("scores", torch.int64)),
                                 ("scores on another device", "scores", on_bad_device("scores")), ("scores one element short", "scores", short_by_one("scores")),
                                 ("scores a column slice of a wider buffer", "scores", column_slice("scores"))])


ROWS_KM = 6

KMEANS_NEAREST_OUT = dict(
    name="kmeans.nearest_on_device(out=)", check=kmeans.check_nearest_out, plain=dict(rows=ROWS_KM), returns=None,
    tensors=lambda dev: dict(out=(zeros(ROWS_KM, torch.float32, dev), zeros(ROWS_KM, torch.int32, dev), zeros(1, torch.int32, dev))),
    accepted=[("out as a list", "out", lambda a, x: list(a["out"]))],
    violations=[("out of two tensors", "out", lambda a, x: a["out"][:2]), ("out holding a list", "out", lambda a, x: (a["out"][0], [0] * ROWS_KM, a["out"][2])),
                ("dist float64", "out", lambda a, x: (a["out"][0].double(), a["out"][1], a["out"][2])), ("dist int32", "out", lambda a, x: (a["out"][0].int(), a["out"][1], a["out"][2])),
                ("dist float16", "out", lambda a, x: (a["out"][0].half(), a["out"][1], a["out"][2])),
                ("which int64", "out", lambda a, x: (a["out"][0], a["out"][1].long(), a["out"][2])), ("which float32", "out", lambda a, x: (a["out"][0], a["out"][1].float(), a["out"][2])),
                ("invalid int64", "out", lambda a, x: (a["out"][0], a["out"][1], a["out"][2].long())), ("invalid of two elements", "out", lambda a, x: (a["out"][0], a["out"][1], zeros(2, torch.int32, x.dev))),
                ("invalid empty", "out", lambda a, x: (a["out"][0], a["out"][1], a["out"][2][:0])),
                ("dist one row short", "out", lambda a, x: (a["out"][0][:-1], a["out"][1], a["out"][2])), ("which one row short", "out", lambda a, x: (a["out"][0], a["out"][1][:-1], a["out"][2])),
                ("dist strided", "out", lambda a, x: (zeros(2 * ROWS_KM, torch.float32, x.dev)[::2], a["out"][1], a["out"][2])),
                ("which strided", "out", lambda a, x: (a["out"][0], zeros(2 * ROWS_KM, torch.int32, x.dev)[::2], a["out"][2])),
                ("dist on another device", "out", lambda a, x: (on_bad_device("d")(dict(d=a["out"][0]), x), a["out"][1], a["out"][2])),
                ("which on another device", "out", lambda a, x: (a["out"][0], on_bad_device("d")(dict(d=a["out"][1]), x), a["out"][2])),
                ("invalid on another device", "out", lambda a, x: (a["out"][0], a["out"][1], on_bad_device("d")(dict(d=a["out"][2]), x)))])


def cpu_entries():
    """Every entry as the CPU file checks it (the GPU file builds its own live-push entries around the handle's state size)."""
    return [HEAD_FORWARD, HEAD_FORWARD_MANY, HEAD_LOSS_GRAD, HEAD_ADAM_STEP_DEV, EMBED_FORWARD, embed_entry(2048), embed_entry(1280), FRONTEND_FORWARD,
            FRONTEND_FORWARD_1D, FRONTEND_STREAM, live_push_entry(1), live_push_entry(2), live_step_entry(1), live_step_entry(2), KMEANS_NEAREST_OUT]


# ---- running an entry ------------------------------------------------------------------------------------------------------------------

def plain_of(entry):
    return entry["plain"]() if callable(entry["plain"]) else dict(entry["plain"])


def arguments(entry, dev, **fill):
    """Fresh well-formed arguments of the entry's tensors (and its integer arguments) on `dev`."""
    a = entry["tensors"](torch.device(dev))
    a.update(fill)
    return a


def changed(entry, case, x, **fill):
    """The well-formed arguments with the case's one change applied (to one argument, or to each of a tuple of them)."""
    a = arguments(entry, x.dev, **fill)
    names = case[1] if isinstance(case[1], tuple) else (case[1],)
    new = {n: case[2](a, x) for n in names}
    a.update(new)
    return a


def exception_of(case):
    return case[3] if len(case) > 3 else ValueError


def call_check(entry, a, dev):
    kw = plain_of(entry)
    if not entry.get("no_device"):
        kw["device"] = torch.device(dev)
    kw.update(entry.get("ints", {}))
    kw.update(a)
    return entry["check"](**kw)


def tensor_parameters(entry):
    """The parameters of the check function that are the caller's tensors: all but its plain ones."""
    names = set(inspect.signature(entry["check"]).parameters)
    return names - set(plain_of(entry)) - set(entry.get("ints", {})) - {"device", "who"}
