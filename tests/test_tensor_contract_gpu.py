"""-m gpu: the tensor contract of the core wrappers on the wrappers themselves.

(a) Every violation of tests/util_tensor_contract.py is given to the wrapper while its library is replaced by tc.HostOnlyLibrary, which
    forwards pure host queries and fails the test on any other call: the refusal is decided before any device call, literally, so no
    refused tensor -- a host pointer, an undersized buffer -- can reach a kernel, whatever the wrapper under test does.  Afterwards the
    well-formed call gives the bits it gave before.
(b) Every accepted variant (strided and sliced inputs, other integer widths, storage one element off a 256-byte boundary, outputs that
    are views inside a canary-filled allocation on a 16-byte boundary and one float past it) gives, with the real library, the bits of
    the plain call on fresh contiguous tensors, and the canaries on both sides of every caller-owned buffer are intact.
(c) EmbeddingModel.forward with B = 7 on handles of max_batch = 3 and a fenced `out` equals the concatenation of three separate calls.

All buffers given to the real library are well-formed."""
import types

import numpy as np
import pytest

from tests import util_tensor_contract as tc

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

CANARY = 0xA5
PAD = 4096             # canary bytes in front of and behind every caller-owned buffer (a multiple of 16)
AVG, SUP, MINC = 100, 500, 2


class Fenced:
    """A caller-owned buffer of `dtype` and `shape` inside a canary-filled allocation, `lead` bytes past a 16-byte boundary."""

    def __init__(self, shape, dtype, lead, dev, fill=None):
        n = int(np.prod(shape)) * torch.empty(0, dtype=dtype).element_size()
        self.whole = torch.full((PAD + lead + n + PAD,), CANARY, dtype=torch.uint8, device=dev)
        assert self.whole.data_ptr() % 16 == 0
        self.lo, self.hi = PAD + lead, PAD + lead + n
        self.view = self.whole[self.lo:self.hi].view(dtype).view(shape)
        assert self.view.data_ptr() % 16 == lead % 16 and self.view.is_contiguous()
        if fill is not None:
            self.view.copy_(fill)

    def intact(self):
        return bool((self.whole[:self.lo] == CANARY).all()) and bool((self.whole[self.hi:] == CANARY).all())


LEADS = (0, 4)          # on a 16-byte boundary, and one float past it (an int64 buffer: 8 bytes past it, the least its dtype allows)


def lead_for(dtype, lead):
    return 8 if lead and dtype == torch.int64 else lead


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def x(dev):
    """The surroundings of the violation tables on the device: the wrong device is the CPU."""
    from multilingual_kws_amd.head import Head
    other, closed = Head(*tc.OTHER_DIMS, max_batch=8, seed=3, device=dev), Head(tc.IN, tc.HID, tc.CLS, max_batch=8, seed=4, device=dev)
    closed.close()
    far = types.SimpleNamespace(in_dim=tc.IN, hidden=tc.HID, classes=tc.CLS, device=torch.device("cuda", 1), h=1)      # (refused before it is looked at)
    yield tc.surroundings(dev, "cpu", other=other, closed=closed, far=far)
    other.close()


@pytest.fixture(scope="module")
def heads(dev):
    from multilingual_kws_amd.head import Head
    hs = [Head(tc.IN, tc.HID, tc.CLS, max_batch=8, seed=s, device=dev) for s in range(3)]
    yield hs
    torch.cuda.synchronize()
    for h in hs:
        h.close()


@pytest.fixture(scope="module")
def blob():
    from multilingual_kws_amd import weights
    return weights.synthetic_blob()


@pytest.fixture(scope="module")
def fe():
    from multilingual_kws_amd.frontend import Frontend
    f = Frontend(max_samples=tc.N_STREAM)
    yield f
    torch.cuda.synchronize()
    f.close()


def clones(*ts):
    return tuple(None if t is None else t.clone() for t in ts)


def same(a, b):
    return len(a) == len(b) and all((p is None and q is None) or (p.dtype == q.dtype and p.shape == q.shape and torch.equal(p, q)) for p, q in zip(a, b))


def refuse_all(entry, run, x, monkeypatch, patch, fill=None, attempt=None):
    """(a) for one entry point.  run(a) -> tuple of result tensors; patch(m, proxy): puts the proxy in place of the wrapper's library;
    attempt(a): the wrapper call alone, where run() prepares something on the device first."""
    from multilingual_kws_amd import _lib
    fill = fill or {}
    before = run(tc.arguments(entry, x.dev, **fill))
    torch.cuda.synchronize()
    proxy = tc.HostOnlyLibrary(_lib.lib())
    cases = [(case, tc.changed(entry, case, x, **fill)) for case in entry["violations"]]          # (built with the real library in place)
    with monkeypatch.context() as m:
        patch(m, proxy)
        for case, a in cases:
            with pytest.raises(tc.exception_of(case)):
                (attempt or run)(a)
            assert proxy.refused == [], (entry["name"], case[0], proxy.refused)
        assert set(proxy.queries) <= tc.HOST_QUERIES
    after = run(tc.arguments(entry, x.dev, **fill))
    torch.cuda.synchronize()
    assert same(before, after), entry["name"]
    return len(cases)


def no_allocation(m):
    """Inside the context a wrapper that allocates (torch.zeros / torch.empty, what they all use) before it refuses fails the test."""
    def refuse(*a, **kw):
        raise AssertionError("a tensor was allocated: a refusal must be decided before anything is allocated")
    m.setattr(torch, "zeros", refuse)
    m.setattr(torch, "empty", refuse)


def patch_module_lib(m, proxy):
    from multilingual_kws_amd import _lib
    m.setattr(_lib, "lib", lambda: proxy)


# ---- the head ------------------------------------------------------------------------------------------------------------------------

def test_head_forward(heads, x, monkeypatch):
    hd = heads[0]
    run = lambda a: (hd.forward(a["emb"]),)
    assert refuse_all(tc.HEAD_FORWARD, run, x, monkeypatch, lambda m, p: m.setattr(hd, "L", p)) >= 8
    plain = run(tc.arguments(tc.HEAD_FORWARD, x.dev))
    assert plain[0].shape == (tc.B_HEAD, tc.CLS) and bool(torch.isfinite(plain[0]).all())
    for case in tc.HEAD_FORWARD["accepted"]:
        assert same(run(tc.changed(tc.HEAD_FORWARD, case, x)), plain), case[0]


def test_head_forward_many(heads, x, monkeypatch):
    from multilingual_kws_amd.head import Head
    entry, fill = tc.HEAD_FORWARD_MANY, dict(heads=heads)
    run = lambda a: (Head.forward_many(a["heads"], a["emb"]),)

    def patch(m, proxy):
        for h in heads + [x.other]:
            m.setattr(h, "L", proxy)
    assert refuse_all(entry, run, x, monkeypatch, patch, fill) >= 13
    emb = tc.arguments(entry, x.dev, **fill)["emb"]
    single = torch.stack([h.forward(emb) for h in heads])
    assert same(run(tc.arguments(entry, x.dev, **fill)), (single,))
    for case in entry["accepted"]:
        a = tc.changed(entry, case, x, **fill)
        want = torch.stack([h.forward(emb) for h in a["heads"]])
        assert same(run(a), (want,)), case[0]


def test_head_loss_grad(heads, x, monkeypatch):
    hd, entry = heads[1], tc.HEAD_LOSS_GRAD

    def run(a):
        stats = hd.loss_grad(a["emb"], a["labels"])
        return clones(stats, hd.grad_view(with_stats=True))
    assert refuse_all(entry, run, x, monkeypatch, lambda m, p: m.setattr(hd, "L", p)) >= 16
    plain = run(tc.arguments(entry, x.dev))
    assert float(plain[0][0]) > 0 and bool(plain[1].abs().sum() > 0)
    for case in entry["accepted"]:
        hd.grad_view(with_stats=True).zero_()
        assert same(run(tc.changed(entry, case, x)), plain), case[0]


def test_head_adam_step_dev(heads, x, monkeypatch):
    hd, entry = heads[2], tc.HEAD_ADAM_STEP_DEV
    p0 = hd.get_params()
    batch = tc.arguments(tc.HEAD_LOSS_GRAD, x.dev)

    def run(a):
        hd.set_params(p0)
        hd.loss_grad(batch["emb"], batch["labels"])
        hd.adam_step_dev(1e-2, a["d_step"])
        return clones(hd.state_view())
    assert refuse_all(entry, run, x, monkeypatch, lambda m, p: m.setattr(hd, "L", p), attempt=lambda a: hd.adam_step_dev(1e-2, a["d_step"])) >= 5
    plain = run(tc.arguments(entry, x.dev))
    assert not np.array_equal(hd.get_params(), p0)
    for case in entry["accepted"]:
        assert same(run(tc.changed(entry, case, x)), plain), case[0]
    hd.set_params(p0)


# ---- the embedding -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("output", ["dense_2", "dense_1", "dense", "global_average_pooling2d"])
def test_embedding_forward(blob, x, monkeypatch, output):
    """Refusals for this value of output=; accepted variants at B = 1, 3 (one chunk) and 7 (chunked, max_batch = 3), each with `out` absent, plain,
    and fenced at both alignments; (c) the chunked call against three separate ones."""
    from multilingual_kws_amd.embedding_model import OUTPUT_LAYERS, EmbeddingModel
    em = EmbeddingModel(blob, max_batch=3, device=x.dev, output=output)
    dim = OUTPUT_LAYERS[output][1]
    try:
        run = lambda a: (em.forward(a["spec"], out=a["out"]),)
        for B in (1, 3, 7):
            entry = tc.embed_entry(dim, B)
            if B >= 3:                                                     # one chunk, and three: `out` one row short would be overrun by the last one
                assert refuse_all(entry, run, x, monkeypatch, lambda m, p: m.setattr(em, "L", p)) >= 15
            a = tc.arguments(entry, x.dev)
            plain = run(a)
            assert plain[0].data_ptr() == a["out"].data_ptr() and plain[0].shape == (B, dim) and bool(torch.isfinite(plain[0]).all()) and bool(plain[0].abs().sum() > 0)
            for case in entry["accepted"]:
                got = run(tc.changed(entry, case, x))[0][:B]
                assert same((got,), plain), (B, case[0])
            fenced_in = Fenced((B, 49, 40), torch.float32, 4, x.dev, fill=a["spec"])
            for lead in LEADS:
                out = Fenced((B, dim), torch.float32, lead, x.dev)
                got = em.forward(fenced_in.view, out=out.view)
                torch.cuda.synchronize()
                assert got.data_ptr() == out.view.data_ptr() and same((got,), plain), (B, lead)
                assert out.intact() and fenced_in.intact(), (B, lead)
            if B == 7:                                                     # (c)
                parts = [em.forward(a["spec"][s:s + 3]) for s in (0, 3, 6)]
                assert [p.shape[0] for p in parts] == [3, 3, 1] and same((torch.cat(parts),), plain)
    finally:
        torch.cuda.synchronize()
        em.close()


# ---- the frontend --------------------------------------------------------------------------------------------------------------------

def patch_frontend(fe):
    def patch(m, proxy):
        m.setattr(fe, "L", proxy)
        patch_module_lib(m, proxy)                 # (frontend.num_frames asks the module's library)
    return patch


def test_frontend_forward(fe, x, monkeypatch):
    entry = tc.FRONTEND_FORWARD
    run = lambda a: (fe.forward(a["audio"], out=a["out"]),)
    assert refuse_all(entry, run, x, monkeypatch, patch_frontend(fe)) >= 16
    assert refuse_all(tc.FRONTEND_FORWARD_1D, run, x, monkeypatch, patch_frontend(fe)) == 1
    a = tc.arguments(entry, x.dev)
    plain = run(a)
    pcm = (a["audio"] * 32768).to(torch.int16)
    plain_pcm = (fe.forward(pcm),)
    assert plain[0].shape == (tc.B_FE, 49, 40) and bool(plain[0].abs().sum() > 0) and bool(plain_pcm[0].abs().sum() > 0)
    for case in entry["accepted"]:
        b = tc.changed(entry, case, x)
        assert same((run(b)[0][:tc.B_FE],), plain_pcm if b["audio"].dtype == torch.int16 else plain), case[0]
    for B in (1, 3):
        assert same((fe.forward(a["audio"][0]),), (plain[0][:1],))                          # the 1-D form
        fenced_in = Fenced((B, tc.CLIP), torch.float32, 4, x.dev, fill=a["audio"][:B])
        fenced_pcm = Fenced((B, tc.CLIP), torch.int16, 2, x.dev, fill=pcm[:B])
        for lead in LEADS:
            out = Fenced((B, 49, 40), torch.float32, lead, x.dev)
            assert same((fe.forward(fenced_in.view, out=out.view),), (plain[0][:B],)) and out.intact() and fenced_in.intact(), (B, lead)
            out = Fenced((B, 49, 40), torch.float32, lead, x.dev)
            assert same((fe.forward(fenced_pcm.view, out=out.view),), (plain_pcm[0][:B],)) and out.intact() and fenced_pcm.intact(), (B, lead)


def test_frontend_stream(fe, x, monkeypatch):
    entry = tc.FRONTEND_STREAM
    run = lambda a: fe.stream(a["audio"], tc.CLIP, tc.HOP, want_raw=True)
    assert refuse_all(entry, run, x, monkeypatch, patch_frontend(fe)) >= 6
    plain = run(tc.arguments(entry, x.dev))
    assert plain[0].shape == (3, 49, 40) and bool(plain[0].abs().sum() > 0)
    for case in entry["accepted"]:
        assert same(run(tc.changed(entry, case, x)), plain), case[0]


def _pushes(fe, audio, h, state, bufs=None):
    """The whole recording pushed h hops at a time -> (every push's spec, raw, meta stacked, the state)."""
    P = audio.numel() // (h * tc.HOP)
    got = []
    for i in range(P):
        new = audio[i * h * tc.HOP:(i + 1) * h * tc.HOP]
        if bufs is None:
            got.append(clones(*fe.live_push(state, new, tc.CLIP, tc.HOP, h, want_raw=True)))
        else:
            for f in bufs:
                f.view.zero_()
            spec, raw, meta = fe.live_push(state, new, tc.CLIP, tc.HOP, h, spec=bufs[0].view, raw=bufs[1].view, meta=bufs[2].view)
            assert spec.data_ptr() == bufs[0].view.data_ptr() and raw.data_ptr() == bufs[1].view.data_ptr() and meta.data_ptr() == bufs[2].view.data_ptr()
            got.append(clones(spec, raw, meta))
    return tuple(torch.stack([g[k] for g in got]) for k in range(3)) + (state,)


@pytest.mark.parametrize("h", [1, 2])
def test_frontend_live_push(fe, x, monkeypatch, h):
    need = fe.L.mkws_frontend_live_state_bytes(fe.h, tc.CLIP, tc.HOP, h)
    assert need > 0 and fe.live_state(tc.CLIP, tc.HOP, h).numel() * 8 >= need
    entry = tc.live_push_entry(h, need)

    def run(a):
        return clones(*fe.live_push(a["state"], a["audio"], tc.CLIP, tc.HOP, h, spec=a["spec"], raw=a["raw"], meta=a["meta"]), a["state"])
    assert refuse_all(entry, run, x, monkeypatch, patch_frontend(fe)) >= 30
    # the accepted variants over a whole recording: 52 hops, the last two (h = 1) or the last one (h = 2) pushes complete windows
    audio = tc.arguments(tc.FRONTEND_STREAM, x.dev)["audio"]
    plain = _pushes(fe, audio, h, fe.live_state(tc.CLIP, tc.HOP, h))
    counts = plain[2][:, 0].tolist()
    assert sum(counts) == 3 and torch.equal(torch.cat([s[:c] for s, c in zip(plain[0], counts)]), fe.stream(audio, tc.CLIP, tc.HOP))
    for case in entry["accepted"]:
        if case[1] == "audio":
            moved = case[2](dict(audio=audio), x)
            assert moved.data_ptr() % 256 == 4
            assert same(_pushes(fe, moved, h, fe.live_state(tc.CLIP, tc.HOP, h)), plain), case[0]
        elif case[1] == "state":
            spare = case[2](tc.arguments(entry, x.dev), x)
            got = _pushes(fe, audio, h, spare)
            assert same(got[:3], plain[:3]) and torch.equal(got[3][:plain[3].numel()], plain[3]) and not bool(got[3][plain[3].numel():].any()), case[0]
    for lead in LEADS:
        bufs = [Fenced((h, 49, 40), torch.float32, lead, x.dev), Fenced((h, 49, 40), torch.int16, lead, x.dev), Fenced((2 + h,), torch.int64, lead_for(torch.int64, lead), x.dev)]
        state = Fenced((plain[3].numel(),), torch.int64, 0, x.dev)
        state.view.zero_()
        got = _pushes(fe, audio, h, state.view, bufs)
        # (rows past a push's count are left as they were: zero in both runs)
        assert same(got, plain), lead
        assert all(f.intact() for f in bufs) and state.intact(), lead


# ---- the live detector ---------------------------------------------------------------------------------------------------------------

def _script(h, dev, windows=24):
    """Scripted probabilities [N, windows, C] that fire in every lane, as pushes of h windows: -> [(probs [N, h, C], meta [2 + h])]."""
    conf = torch.tensor([0.1, 0.9, 0.95, 0.9, 0.8, 0.2, 0.1, 0.1, 0.85, 0.9, 0.9, 0.3] * 2, dtype=torch.float32)[:windows]
    probs = torch.stack([torch.stack([1 - c, torch.zeros_like(c), c], -1) for c in (conf, conf.roll(3))]).to(dev)
    times = [20 * w for w in range(windows)]
    return [(probs[:, w:w + h].contiguous(), torch.tensor([h, w] + times[w:w + h], dtype=torch.int64, device=dev)) for w in range(0, windows, h)]


def _steps(script, h, state, d_thr, bufs=None):
    from multilingual_kws_amd import detector
    got = []
    for probs, meta in script:
        if bufs is None:
            out, scores = None, torch.zeros((tc.N_DET, h), dtype=torch.float64, device=probs.device)
        else:
            out, scores = bufs[0].view, bufs[1].view
            out.zero_()
            scores.zero_()
        words = detector.detect_live_step(state, probs, meta, d_thr, AVG, SUP, MINC, tc.HISTORY, out=out, scores=scores)
        got.append(clones(words, scores))
    return torch.stack([g[0] for g in got]), torch.stack([g[1] for g in got]), state


@pytest.mark.parametrize("h", [1, 2])
def test_detect_live_step(x, monkeypatch, h):
    from multilingual_kws_amd import detector
    entry = tc.live_step_entry(h)

    def run(a):
        out = detector.detect_live_step(a["state"], a["probs"], a["meta"], a["d_thresholds"], AVG, SUP, MINC, tc.HISTORY, out=a["out"], scores=a["scores"])
        return clones(out, a["scores"], a["state"])
    assert refuse_all(entry, run, x, monkeypatch, patch_module_lib) >= 28
    a = tc.arguments(entry, x.dev)
    script, d_thr = _script(h, x.dev), a["d_thresholds"]
    plain = _steps(script, h, detector.live_detector_state(tc.N_DET, tc.T_DET, tc.HISTORY, device=x.dev), d_thr)
    counts = sum(detector.live_unpack(w.cpu().numpy(), tc.N_DET, tc.T_DET, h)[0].astype(np.int64) for w in plain[0])
    assert counts.min() >= 1, "the scripted stream must leave events in every lane"
    spare = _steps(script, h, torch.zeros(plain[2].numel() + 5, dtype=torch.int64, device=x.dev), d_thr)
    assert same(spare[:2], plain[:2]) and torch.equal(spare[2][:plain[2].numel()], plain[2]) and not bool(spare[2][plain[2].numel():].any())
    longer = [(p, torch.cat([m, torch.full((3,), -1, dtype=torch.int64, device=x.dev)])) for p, m in script]
    assert same(_steps(longer, h, torch.zeros_like(plain[2]), d_thr), plain)
    for lead in LEADS:
        bufs = [Fenced((detector.live_out_words(tc.N_DET, tc.T_DET, h),), torch.int64, lead_for(torch.int64, lead), x.dev),
                Fenced((tc.N_DET, h), torch.float64, lead_for(torch.int64, lead), x.dev)]
        state = Fenced((plain[2].numel(),), torch.int64, lead_for(torch.int64, lead), x.dev)
        state.view.zero_()
        thr = Fenced((tc.T_DET,), torch.float64, lead_for(torch.int64, lead), x.dev, fill=d_thr)
        assert same(_steps(script, h, state.view, thr.view, bufs), plain), lead
        assert all(f.intact() for f in bufs + [state, thr]), lead


# ---- holes the audit found ---------------------------------------------------------------------------------------------------------------

def test_kmeans_nearest_out(x, monkeypatch):
    from multilingual_kws_amd import kmeans
    entry = tc.KMEANS_NEAREST_OUT
    pts = tc.rand((tc.ROWS_KM, 32), x.dev, 7)
    group = torch.tensor([0, 1, 0, 1, 1, 0], dtype=torch.int32, device=x.dev)
    centers = tc.rand((2, 3, 32), x.dev, 8)
    run = lambda a: clones(*kmeans.nearest_on_device(pts, group, centers, out=a["out"]))
    assert refuse_all(entry, run, x, monkeypatch, patch_module_lib) >= 15
    plain = clones(*kmeans.nearest_on_device(pts, group, centers))
    want = kmeans.nearest_host(pts.cpu().numpy(), centers[0].cpu().numpy())[1]
    assert int(plain[2][0]) == 0 and plain[1].tolist()[0] == int(want[0]) and bool(torch.isfinite(plain[0]).all())
    for lead in LEADS:
        bufs = [Fenced((tc.ROWS_KM,), torch.float32, lead, x.dev), Fenced((tc.ROWS_KM,), torch.int32, lead, x.dev), Fenced((1,), torch.int32, lead, x.dev)]
        bufs[2].view.zero_()
        got = kmeans.nearest_on_device(pts, group, centers, out=tuple(f.view for f in bufs))
        assert same(got, plain) and all(f.intact() for f in bufs), lead


def test_many_stream_wrappers_refuse_host_tensors_before_any_device_call(fe, x, monkeypatch):
    """The state tensor (and every caller-supplied output) of the many-stream calls on the host, or of another dtype: shapes and strides
    are right, so only the device / dtype rule can refuse them."""
    from multilingual_kws_amd import _lib, detector
    from multilingual_kws_amd.resample import Resampler
    S, h = 2, 1
    states = fe.live_state_many(S, tc.CLIP, tc.HOP, h, device=x.dev)
    audio = tc.rand((S, h * tc.HOP), x.dev, 9)
    good = dict(spec=torch.zeros((S * h, 49, 40), device=x.dev), raw=torch.zeros((S * h, 49, 40), dtype=torch.int16, device=x.dev),
                meta=torch.zeros((S, 2 + h), dtype=torch.int64, device=x.dev), active=torch.ones(S, dtype=torch.int32, device=x.dev))
    rs = Resampler(48000)
    rs_states, rs_audio = rs.live_state_many(S, device=x.dev), tc.rand((S, rs.live_in_samples(tc.HOP)), x.dev, 10)
    N, T = tc.N_DET, tc.T_DET
    d_states = detector.live_detector_state_many(S, N, T, tc.HISTORY, device=x.dev)
    d_probs, d_meta = torch.zeros((N, S * h, 3), device=x.dev), torch.zeros((S, 2 + h), dtype=torch.int64, device=x.dev)
    d_thr = torch.tensor([0.3, 0.5, 0.7], dtype=torch.float64, device=x.dev)
    d_out, d_scores = torch.zeros(detector.live_out_words_many(S, N, T, h), dtype=torch.int64, device=x.dev), torch.zeros((S, N, h), dtype=torch.float64, device=x.dev)
    r_states = detector.live_detector_state_routes(S, T, tc.HISTORY, device=x.dev)
    r_probs, r_slot, r_thr = torch.zeros((S * h, 3), device=x.dev), torch.zeros(S, dtype=torch.int32, device=x.dev), d_thr.repeat(S, 1)
    r_out, r_scores = torch.zeros(detector.live_out_words_routes(S, T, h), dtype=torch.int64, device=x.dev), torch.zeros((S, h), dtype=torch.float64, device=x.dev)
    hi = tc.rand((2, 960), x.dev, 12)                                     # Resampler.forward(out=): rows that overlap, another dtype, the host
    n_out = rs.out_samples(960)
    rs_good_out = torch.zeros((2, n_out), device=x.dev)
    want_rs = rs.forward(hi, out=rs_good_out).clone()
    bad = dict(overlap=torch.zeros(2 * n_out, device=x.dev).as_strided((2, n_out), (n_out - 1, 1)), host=torch.zeros((2, n_out)),
               f64=torch.zeros((2, n_out), dtype=torch.float64, device=x.dev), strided_thr=torch.zeros(2 * T, dtype=torch.float64, device=x.dev)[::2],
               rs_out_host=torch.zeros((S, tc.HOP)), active_host=torch.ones(S, dtype=torch.int32), states_host=states.cpu(), rs_states_host=rs_states.cpu(),
               d_states_host=d_states.cpu())
    proxy = tc.HostOnlyLibrary(_lib.lib())
    push = lambda **kw: fe.live_push_many(kw.pop("states", states), audio, tc.CLIP, tc.HOP, h, **dict(good, **kw))
    step = lambda **kw: detector.detect_live_step_many(kw.pop("states", d_states), d_probs, kw.pop("meta", d_meta), kw.pop("d_thresholds", d_thr), AVG, SUP, MINC, tc.HISTORY,
                                                       out=kw.pop("out", d_out), scores=kw.pop("scores", d_scores))
    route = lambda **kw: detector.detect_live_step_routes(kw.pop("states", r_states), r_probs, d_meta, r_slot, r_thr, AVG, SUP, MINC, tc.HISTORY,
                                                          out=kw.pop("out", r_out), scores=kw.pop("scores", r_scores))
    with monkeypatch.context() as m:
        m.setattr(fe, "L", proxy)
        m.setattr(rs, "L", proxy)
        patch_module_lib(m, proxy)
        no_allocation(m)
        calls = [lambda: fe.live_push_many(bad["states_host"], audio, tc.CLIP, tc.HOP, h),                 # (defaults: nothing may be allocated first)
                 lambda: fe.live_push_many(bad["states_host"], audio, tc.CLIP, tc.HOP, h, want_raw=True),
                 lambda: rs.live_push_many(bad["rs_states_host"], rs_audio, tc.HOP),
                 lambda: detector.detect_live_step_many(bad["d_states_host"], d_probs, d_meta, d_thr, AVG, SUP, MINC, tc.HISTORY),
                 lambda: step(d_thresholds=bad["strided_thr"]),
                 lambda: rs.forward(hi, out=bad["overlap"]), lambda: rs.forward(hi, out=bad["host"]), lambda: rs.forward(hi, out=bad["f64"]),
                 lambda: push(states=states.cpu()), lambda: push(spec=good["spec"].cpu()), lambda: push(spec=good["spec"].double()), lambda: push(raw=good["raw"].cpu()),
                 lambda: push(raw=good["raw"].int()), lambda: push(meta=good["meta"].cpu()), lambda: push(meta=good["meta"].int()), lambda: push(active=good["active"].cpu()),
                 lambda: rs.live_push_many(rs_states.cpu(), rs_audio, tc.HOP), lambda: rs.live_push_many(rs_states, rs_audio, tc.HOP, out=bad["rs_out_host"]),
                 lambda: rs.live_push_many(rs_states, rs_audio, tc.HOP, active=bad["active_host"]),
                 lambda: step(states=d_states.cpu()), lambda: step(meta=d_meta.cpu()), lambda: step(d_thresholds=d_thr.cpu()), lambda: step(out=d_out.cpu()),
                 lambda: step(scores=d_scores.cpu()), lambda: step(out=d_out.double()), lambda: step(scores=d_scores.float()),
                 lambda: route(states=r_states.cpu()), lambda: route(out=r_out.cpu()), lambda: route(scores=r_scores.cpu())]
        for k, call in enumerate(calls):
            with pytest.raises(ValueError):
                call()
            assert proxy.refused == [], k
    # and the same well-formed calls go through
    push()
    rs.live_push_many(rs_states, rs_audio, tc.HOP)
    step()
    route()
    fe.live_push_many(states, audio, tc.CLIP, tc.HOP, h, want_raw=True)
    detector.detect_live_step_many(d_states, d_probs, d_meta, d_thr, AVG, SUP, MINC, tc.HISTORY)
    spaced = torch.zeros((2, n_out + 3), device=x.dev)[:, :n_out]                                # rows apart: accepted, the same bits
    assert torch.equal(rs.forward(hi, out=spaced), want_rs) and torch.equal(rs.forward(hi, out=rs_good_out), want_rs)
    torch.cuda.synchronize()
    rs.close()


def test_training_wrappers_refuse_what_their_kernels_would_misread(blob, x, monkeypatch):
    from multilingual_kws_amd import _lib
    from multilingual_kws_amd.embedding_trainer import EmbeddingTrainer
    from multilingual_kws_amd.train_multilingual_embedding import LogitsLayer
    lay = LogitsLayer(4, device=x.dev, seed=1)
    emb, labels = tc.rand((5, 1024), x.dev, 11), torch.tensor([0, 1, 2, 3, 1], dtype=torch.int64, device=x.dev)
    stats, d_emb = lay.loss_grad(emb, labels)
    before = clones(stats, d_emb, lay.forward(emb))
    tr = EmbeddingTrainer(blob, device=x.dev)
    # a training-mode forward with the caller's keep scales: contiguous, and as a strided view (made contiguous by the wrapper) -- the same bits
    B, block = 2, "2b"
    spec = tc.arguments(tc.embed_entry(1024, B), x.dev)["spec"]
    scale = torch.tensor([1.25, 0.0], dtype=torch.float32, device=x.dev)
    want_emb = tr.forward_train(spec, keep_scales={block: scale}).clone()
    assert not torch.equal(want_emb, tr.forward_train(spec).clone()), "the block must be a residual one: its keep scale matters"
    got_emb = tr.forward_train(spec, keep_scales={block: torch.stack([scale, scale], 1)[:, 0]}).clone()
    assert torch.equal(got_emb, want_emb) and bool(torch.isfinite(want_emb).all())
    wrong = [torch.zeros((2, 49, 41), device=x.dev), torch.zeros((2, 40, 49), device=x.dev), torch.zeros((B - 1, 1024), device=x.dev),
             torch.zeros((B + 1, 1024), device=x.dev), torch.zeros((B, 1023), device=x.dev), torch.zeros(B * 1024, device=x.dev),
             scale.double(), scale[:1], torch.cat([scale, scale]), scale.cpu()]
    proxy = tc.HostOnlyLibrary(_lib.lib())
    with monkeypatch.context() as m:
        m.setattr(lay, "L", proxy)
        m.setattr(tr, "L", proxy)
        for call in (lambda: tr.backward(wrong[2]), lambda: tr.backward(wrong[3]), lambda: tr.backward(wrong[4]), lambda: tr.backward(wrong[5]),
                     lambda: tr.forward_train(spec, keep_scales={block: wrong[6]}), lambda: tr.forward_train(spec, keep_scales={block: wrong[7]}),
                     lambda: tr.forward_train(spec, keep_scales={block: wrong[8]}), lambda: tr.forward_train(spec, keep_scales={block: wrong[9]}),
                     lambda: tr.forward_train(spec, drop_masks={block: [True]}), lambda: tr.forward_train(spec, drop_masks={block: [True] * 3}),
                     lambda: lay.forward(emb.double()), lambda: lay.forward(emb.cpu()), lambda: lay.forward(emb[:, :512]), lambda: lay.loss_grad(emb, labels.cpu()),
                     lambda: lay.loss_grad(emb, labels[:4]), lambda: lay.loss_grad(emb, labels.float()), lambda: lay.loss_grad(emb.half(), labels),
                     lambda: tr.forward_train(wrong[0]), lambda: tr.forward_train(wrong[1])):
            with pytest.raises(ValueError):
                call()
            assert proxy.refused == []
    stats, d_emb = lay.loss_grad(tc.column_slice("emb")(dict(emb=emb), x), labels.to(torch.int32))
    assert same(clones(stats, d_emb, lay.forward(emb)), before)
    tr.backward(torch.ones((B, 1024), device=x.dev))                       # the tape of the last forward_train is still there: the refusals left it alone
    assert bool(torch.isfinite(tr.grads).all()) and bool(tr.grads.abs().sum() > 0)
    torch.cuda.synchronize()
