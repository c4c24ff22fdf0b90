"""-m gpu: the embedding forward on BOTH sides of every handle size at which mkws_embed_create's plan changes.

tests/util_embed_plan.py restates the per-handle plan rules; boundaries(CU count) lists the handle sizes n whose plan differs from that of
n - 1.  One case per edge builds the default-option handles of n - 1 and n clips and holds each to
  * the restatement: options read back (block_tiles, fuse_cluster, fuse_cluster_chain, fuse_gemv, fuse_mid), the presence of the cluster
    exchange buffers (does set_option("fuse_cluster", 1) succeed), and the WHOLE (stage, kernel) sequence mkws_embed_profile reports -- tile
    shapes, GEMV rows, clips per workgroup, split-K folds.  The two sequences differ exactly where the restatement says, so a case proves it
    straddles an edge.  (Two rules leave no trace in a kernel name -- block 2a's channel-block walk from 128 clips and the stem grid: for
    those the restatement and the numbers below are all there is);
  * the oracle (float32 PyTorch-CPU EmbeddingOracle, run once on 61 clips) at the FULL batch B = max_batch, every row, at the bounds of
    tests/test_embedding_gpu.py: 1e-4 relative on ordinary clips, 1e-3 on the silent and the uniformly loud one, the element-wise
    1e-3 |b| + 2e-5 max|b| of test_full_batch_properties, equal argmax.  Row r holds clip r % 61 (61 is prime: every workgroup slot, pair
    half and row tile meets every clip);
  * taps at the full batch of the stages whose kernel changes at the edge (ragged last row tile of that tile shape, last workgroup);
  * rows never interact: sub-batches are bit-equal to the rows of the full batch;
  * guard bands: a second handle of the same size under MKWS_EMBED_GUARD=4096 on fenced input / output buffers, bit-equal to the plain one
    at the full and at a ragged batch, no guard word touched, pads intact.
Further cases: 1025 and 2048 clips (every kernel takes several rounds of workgroups; the paired kernels for the first time), the cluster
kernel set by option on 33- and 64-clip handles, plan_batch on a 256-clip handle, and the stand-alone top conv's 2x2 tile (fuse_top = 0)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import util_embed_plan as up  # noqa: E402
from test_embedding_gpu import REL_TOL, _rel, _spec, _within  # noqa: E402
from test_guard_bands_gpu import CANARY, _fenced, _pads_intact  # noqa: E402

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

NCLIPS = 61
SILENT, LOUD = 3, 4
MAX_ROWS = 2048
# The parametrisation is that of a 256-CU device (MI355X); on another CU count the same sizes are run against that device's restatement, and
# test_edges_only_another_cu_count_has adds the edges it has besides.
EDGES_256 = [n for n, _ in up.boundaries(256, upto=MAX_ROWS)]
# every handle size this file creates (tests/test_embed_plan_cpu.py: each lies directly on one side of an edge)
HANDLE_SIZES = sorted({m for n in EDGES_256 for m in (n - 1, n)} | {1025, 33, 64, 65, 256})


@pytest.fixture(scope="module")
def ctx():
    from multilingual_kws_amd import weights
    from oracle.efficientnet_oracle import EmbeddingOracle
    blob = weights.synthetic_blob()
    rng = np.random.default_rng(61)
    spec = _spec(rng, NCLIPS)
    spec[SILENT] = 0.0
    spec[LOUD] = (rng.integers(500, 671, size=(49, 40)) * np.float32(10 / 256))
    taps = {}
    ref = EmbeddingOracle(blob).forward(spec, taps).numpy()
    taps = {k: v.reshape(NCLIPS, -1) for k, v in taps.items()}
    dev = torch.device("cuda:0")
    clip = np.arange(MAX_ROWS) % NCLIPS
    x = torch.from_numpy(spec[clip]).to(dev)
    return dict(blob=blob, dev=dev, cus=torch.cuda.get_device_properties(dev).multi_processor_count, ref=ref, taps=taps, x=x, clip=clip,
                ordinary=(clip != SILENT) & (clip != LOUD))


def _against_oracle(got, want, ordinary, what, floor=1e-5):
    special = ~ordinary
    print(what, "rel ordinary %.3g" % _rel(got[ordinary], want[ordinary]), "special %.3g" % (_rel(got[special], want[special]) if special.any() else 0.0))
    assert _rel(got[ordinary], want[ordinary]) < REL_TOL, what
    if special.any():
        assert _rel(got[special], want[special]) < 1e-3, what
    return _within(got[ordinary], want[ordinary], floor=floor)


def _handles(ctx, n, opts, monkeypatch):
    from multilingual_kws_amd.embedding_model import EmbeddingModel
    assert n in HANDLE_SIZES or ctx["cus"] != 256, n
    plain = EmbeddingModel(ctx["blob"], max_batch=n)
    monkeypatch.setenv("MKWS_EMBED_GUARD", "4096")
    guarded = EmbeddingModel(ctx["blob"], max_batch=n)
    monkeypatch.delenv("MKWS_EMBED_GUARD")
    assert plain.get_option("guard_floats") == 0 and guarded.get_option("guard_floats") == 4096 and guarded.get_option("guard_bands") >= 15
    for em in (plain, guarded):
        for k, v in opts.items():
            em.set_option(k, v)
    return plain, guarded


def _sequence(em, x, probe_ok):
    seq = [[s, k] for s, k, _ in em.profile(x, reps=1)]
    return seq if probe_ok else [r for r in seq if r[0] in up.PROBE_FREE_STAGES]


def _check_class(em, p, n, x, fuse_top, default_options):
    """The handle runs the plan p: options read back, and the launch sequence of its full batch.  -> (the sequence, the restatement's)"""
    probe_ok = em.get_option("fuse_pair") == 1
    if default_options:
        assert em.get_option("block_tiles") == p["block_tiles"], n
        assert em.get_option("fuse_mid") == p["fuse_mid"], n
        assert em.get_option("fuse_gemv") == 1, n                         # the switch is on for every handle: launch_gemm takes the kernel on the planned rows
        assert em.get_option("fuse_cluster") == (p["fuse_cluster"] if probe_ok else 0), n
        assert em.get_option("fuse_cluster_chain") == (p["fuse_cluster_chain"] if probe_ok else 0), n
        # the exchange buffers exist <=> the option can be set (and is put back)
        from multilingual_kws_amd._lib import MkwsError
        was = em.get_option("fuse_cluster")
        if p["cluster_buffers"]:
            em.set_option("fuse_cluster", 1)
        else:
            with pytest.raises(MkwsError):
                em.set_option("fuse_cluster", 1)
        em.set_option("fuse_cluster", was)
    want = up.launches(p, n, fuse_top=fuse_top)
    if not probe_ok:
        want = [r for r in want if r[0] in up.PROBE_FREE_STAGES]
    got = _sequence(em, x[:n], probe_ok)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, (n, i, g, w)
    assert len(got) == len(want), (n, got[len(want):], want[len(got):])
    return got, want


def _check_numbers(ctx, plain, guarded, n, taps):
    """Oracle at the full batch (embedding and taps), sub-batches, guard bands."""
    x, clip, ordinary = ctx["x"][:n], ctx["clip"][:n], ctx["ordinary"][:n]
    full = plain.forward(x)
    got, want = full.cpu().numpy(), ctx["ref"][clip]
    assert np.isfinite(got).all()
    _against_oracle(got, want, ordinary, (n, "embedding"))
    assert _within(got, want, floor=2e-5), n
    assert np.array_equal(got.argmax(1), want.argmax(1)), n
    for name in taps:
        t = plain.tap(x, name).cpu().numpy().reshape(n, -1)
        assert _against_oracle(t, ctx["taps"][name][clip], ordinary, (n, name)), (n, name)
    for b in sorted({b for b in (1, 2, 3, n // 2 + 1, n - 3, n - 1) if 1 <= b < n}):
        assert torch.equal(plain.forward(x[:b]), full[:b]), (n, b)
    win, sview = _fenced(n * 1960)
    wout, eview = _fenced(n * 1024)
    sview.copy_(x.reshape(-1))
    for b in sorted({n, max(1, n // 2 - 1)}, reverse=True):
        eview.view(torch.int32).fill_(CANARY)
        for rep in range(2):                     # a repeated call: flags / generation counters of the exchange kernels
            out = guarded.forward(sview[:b * 1960].view(b, 49, 40), out=eview[:b * 1024].view(b, 1024))
            torch.cuda.synchronize()
            assert torch.equal(out, full[:b]), (n, b, "results depend on memory outside the buffers")
        assert bool((eview.view(torch.int32)[b * 1024:] == CANARY).all()), (n, b, "a store behind the batch's rows")
        assert _pads_intact(wout, n * 1024) and _pads_intact(win, n * 1960), (n, b)
        assert guarded.get_option("guard_violations") == 0, (n, b)


def _check_handle(ctx, monkeypatch, n, p, taps, opts=None, fuse_top=1):
    opts = dict(opts or {})
    if not fuse_top:
        opts["fuse_top"] = 0
    plain, guarded = _handles(ctx, n, opts, monkeypatch)
    try:
        seqs = _check_class(plain, p, n, ctx["x"], fuse_top, default_options=not (set(opts) - {"fuse_top"}))
        _check_numbers(ctx, plain, guarded, n, taps)
        assert plain.get_option("pair_degraded") == 0 and guarded.get_option("pair_degraded") == 0, n
    finally:
        plain.close()
        guarded.close()
    return seqs


def _check_edge(ctx, monkeypatch, lo, hi, fuse_top=1):
    cus = ctx["cus"]
    plo, phi = up.plan(lo, cus), up.plan(hi, cus)
    changed = [k for k in up.plan_class(hi, cus) if plo[k] != phi[k]]
    taps = up.taps_of(changed)
    got_lo, want_lo = _check_handle(ctx, monkeypatch, lo, plo, taps, fuse_top=fuse_top)
    got_hi, want_hi = _check_handle(ctx, monkeypatch, hi, phi, taps, fuse_top=fuse_top)
    # the case straddles an edge: the two launch sequences differ in the stages the restatement names (cluster_buffers, fuse_walk and
    # stem_walks show in no kernel name; tests/test_embed_plan_cpu.py ties the stages to the keys that change)
    assert up.stages_that_differ(got_lo, got_hi) == up.stages_that_differ(want_lo, want_hi), (lo, hi)


@pytest.mark.parametrize("n", [n for n in EDGES_256 if n not in (409, 2048)])
def test_both_sides_of_an_edge(ctx, monkeypatch, n):
    _check_edge(ctx, monkeypatch, n - 1, n)


def test_edges_only_another_cu_count_has(ctx, monkeypatch):
    for n, _ in up.boundaries(ctx["cus"], upto=MAX_ROWS):
        if n not in EDGES_256:
            _check_edge(ctx, monkeypatch, n - 1, n)


def test_standalone_top_conv_edge(ctx, monkeypatch):
    """409 clips: the stand-alone top conv's tile goes from 1x2 to 2x2.  Handles above 32 clips launch it only with fuse_top = 0 (or without
    the paired chain): run that way, with `top` (plain epilogue) and `gap` (pooling epilogue) tapped."""
    assert up.plan(408, 256)["top"] != up.plan(409, 256)["top"]
    _check_edge(ctx, monkeypatch, 408, 409, fuse_top=0)


def test_first_size_above_1024(ctx, monkeypatch):
    """1025 clips: the last plan class below 2048 (that of 1024), and the first handle whose paired kernels take more than one round of
    workgroups (136 pairs = 272 workgroups on 256 CUs)."""
    cus = ctx["cus"]
    assert up.plan_class(1025, cus) == up.plan_class(2047, cus)
    _check_handle(ctx, monkeypatch, 1025, up.plan(1025, cus), up.taps_of(["dense", "block_tiles", "pair_mt", "stem_walks"]))


@pytest.mark.parametrize("n", [2047, 2048])
def test_edge_at_2048(ctx, monkeypatch, n):
    """2048 clips: all three dense layers on the 2x4 tile; 2047: the last handle of the 1x4 class.  One handle per case (a gigabyte of workspace each)."""
    cus = ctx["cus"]
    assert up.plan_class(2047, cus) != up.plan_class(2048, cus)
    _check_handle(ctx, monkeypatch, n, up.plan(n, cus), up.taps_of(["dense", "dense_2", "block_tiles", "pair_mt"]))


@pytest.mark.parametrize("n", [33, 64])
def test_cluster_kernel_by_option(ctx, monkeypatch, n):
    """Handles of 33 .. 64 clips own cluster exchange buffers and take the cluster kernel by option: 33 clips leave a ragged last cluster on
    both image sizes (1 clip per cluster on 4x3 images, 4 on 2x2), 64 is the largest such handle."""
    from multilingual_kws_amd.embedding_model import EmbeddingModel
    probe = EmbeddingModel(ctx["blob"], max_batch=n)
    ok = probe.get_option("fuse_pair") == 1
    probe.close()
    if not ok:
        pytest.skip("dispatch probe failed on this device: the cluster kernel is not in use")
    p = up.plan(n, ctx["cus"])
    assert p["fuse_cluster"] == 0 and p["cluster_buffers"] == 1
    p["fuse_cluster"] = 1
    _check_handle(ctx, monkeypatch, n, p, up.TAPS_OF_KEY["fuse_cluster"], opts={"fuse_cluster": 1})


def test_cluster_kernel_refused_above_64(ctx):
    from multilingual_kws_amd._lib import MkwsError
    from multilingual_kws_amd.embedding_model import EmbeddingModel
    em = EmbeddingModel(ctx["blob"], max_batch=65)
    try:
        with pytest.raises(MkwsError):
            em.set_option("fuse_cluster", 1)
        assert em.get_option("fuse_cluster") == 0
    finally:
        em.close()


def test_plan_batch_follows_the_restatement(ctx):
    """Option plan_batch on a 256-clip handle (serving lanes): the tiny-image kernels take the workgroup shapes of the planned size -- 257: two
    clips per 4x3 workgroup, 513: 8-clip pairs, 1021: four clips --, the GEMM tiles stay those of 256 clips, the numbers stay the oracle's,
    and plan_batch = 0 restores the first result bit for bit."""
    from multilingual_kws_amd.embedding_model import EmbeddingModel
    cus, n = ctx["cus"], 256
    x, clip, ordinary = ctx["x"][:n], ctx["clip"][:n], ctx["ordinary"][:n]
    want = ctx["ref"][clip]
    em = EmbeddingModel(ctx["blob"], max_batch=n)
    try:
        probe_ok = em.get_option("fuse_pair") == 1
        first = em.forward(x).clone()
        seen = set()
        for pb in (257, 513, 1021):
            em.set_option("plan_batch", pb)
            p = up.plan(n, cus)
            q = up.plan(pb, cus)
            p.update({k: q[k] for k in ("block_tiles", "pair_mt", "mid4a_clips")})
            seen.add((p["block_tiles"], p["pair_mt"]))
            assert em.get_option("plan_batch") == pb and em.get_option("block_tiles") == p["block_tiles"], pb
            exp = up.launches(p, n)
            got = _sequence(em, x, probe_ok)
            assert got == (exp if probe_ok else [r for r in exp if r[0] in up.PROBE_FREE_STAGES]), (pb, got)
            if probe_ok:
                assert ["chain:6b,6c,6d,7a,top", "mbconv_pair_chain_kernel<%d,8>" % up.pair_row_tiles(pb, cus)] in got, pb
            out = em.forward(x).cpu().numpy()
            _against_oracle(out, want, ordinary, ("plan_batch", pb))
            assert _within(out, want, floor=2e-5) and np.array_equal(out.argmax(1), want.argmax(1)), pb
            for name in ("block4a", "block6a", "block7a"):
                t = em.tap(x, name).cpu().numpy().reshape(n, -1)
                assert _against_oracle(t, ctx["taps"][name][clip], ordinary, ("plan_batch", pb, name)), (pb, name)
        if cus == 256:
            assert seen == {(2, 1), (2, 2), (3, 2)}
        em.set_option("plan_batch", 0)
        assert em.get_option("plan_batch") == n and em.get_option("block_tiles") == up.block43_row_tiles(n, cus)
        assert torch.equal(em.forward(x), first)
    finally:
        em.close()
