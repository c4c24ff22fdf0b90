"""-m gpu: the HIP embedding forward against the PyTorch-CPU oracle, stage by stage, through the C-ABI.
Tolerance: north_star asks for 1e-3 relative (fp32); measured error is ~1e-6, asserted at 1e-4."""
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
REL_TOL = 1e-4


@pytest.fixture(scope="module")
def ctx():
    from multilingual_kws_amd import weights
    from multilingual_kws_amd.embedding_model import EmbeddingModel
    from oracle.efficientnet_oracle import EmbeddingOracle
    blob = weights.synthetic_blob()
    return dict(blob=blob, em=EmbeddingModel(blob, max_batch=1024), oracle=EmbeddingOracle(blob), dev=torch.device("cuda:0"))


def _rel(a, b):
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-30))


def _within(a, b, rtol=1e-3, floor=1e-5):
    """north_star's tolerance taken literally, element by element: |a - b| <= 1e-3 |b| + 1e-5 max|b| (the floor keeps elements that
    are ~0 next to O(1) neighbours from asking for more digits than fp32 accumulation has)."""
    return bool((np.abs(a - b) <= rtol * np.abs(b) + floor * np.abs(b).max()).all())


def _spec(rng, n):
    return (rng.integers(0, 670, size=(n, 49, 40)).astype(np.float32) * np.float32(10 / 256))


def test_every_stage_matches_oracle(ctx):
    rng = np.random.default_rng(0)
    spec = _spec(rng, 5)
    spec[3] = 0.0                      # an all-silent clip
    spec[4] = (rng.integers(500, 671, size=(49, 40)) * np.float32(10 / 256))     # a uniformly loud clip
    taps = {}
    ref = ctx["oracle"].forward(spec, taps).numpy()
    x = torch.from_numpy(spec).to(ctx["dev"])
    assert len(taps) == 69
    for name, exp in taps.items():
        got = ctx["em"].tap(x, name).cpu().numpy().reshape(exp.shape)
        assert _rel(got[:3], exp[:3]) < REL_TOL, name            # ordinary clips: fp32-roundoff class
        assert _rel(got[3:], exp[3:]) < 1e-3, name               # silent / loud clips: north_star tolerance
        assert _within(got[:3], exp[:3]), name                   # ... and the literal element-wise form of it
    emb = ctx["em"].forward(x).cpu().numpy()
    assert emb.shape == (5, 1024) and _rel(emb[:3], ref[:3]) < REL_TOL and _rel(emb, ref) < 1e-3
    assert _within(emb, ref)
    assert np.array_equal(emb.argmax(1), ref.argmax(1))
    assert np.array_equal(ctx["em"].predict(spec[..., None]), emb)          # Keras-style numpy API, NHWC input


def test_execution_options_agree(ctx):
    """fuse_front / fuse_block / fuse_mid / fuse_back / fuse_pair are A/B switches: every combination must match the oracle."""
    spec = _spec(np.random.default_rng(12), 9)
    x = torch.from_numpy(spec).to(ctx["dev"])
    ref = ctx["oracle"].forward(spec).numpy()
    try:
        for combo, (front, block, mid, pair) in enumerate(((0, 0, 0, 0), (1, 0, 0, 1), (1, 2, 1, 1), (0, 2, 0, 0), (1, 1, 2, 1), (0, 0, 1, 0), (1, 2, 1, 0))):
            ctx["em"].set_option("fuse_chain", combo & 1)          # the depth-fused chain only exists on top of fuse_block = 2
            ctx["em"].set_option("fuse_pair", pair)
            ctx["em"].set_option("fuse_front", front)
            ctx["em"].set_option("fuse_block", block)
            ctx["em"].set_option("fuse_mid", mid)
            ctx["em"].set_option("fuse_walk", (combo >> 1) & 1)    # 2a's front kernel: one workgroup per clip walking the channel blocks, or one per block
            ctx["em"].set_option("fuse_se4", (combo >> 2) & 1)     # 4x3-image blocks: squeeze-excite on the 4x4x1 instruction + gate applied in place, or 16x16x4 streams + gate pass
            ctx["em"].set_option("fuse_back", 1 if mid != 2 else 0)
            ctx["em"].set_option("fuse_stem", front)
            ctx["em"].set_option("fuse_gap", front)
            assert _rel(ctx["em"].forward(x).cpu().numpy(), ref) < REL_TOL, (front, block, mid, pair)
            for name in ("stem", "block1a_dw", "block1a_gate", "block1a", "block2a_dw", "block2a_gate", "block2a", "block2b_dw", "block2b", "block3a_gate",
                         "block2b_gate", "block3a", "block3b_dw", "block3b_gate", "block3b", "block4a", "block4c_dw", "block4c", "block5b_dw", "block5b_gate", "block6a", "block6b", "block6c_dw", "block6c_gate", "block6d", "block7a_dw", "block7a", "top", "gap"):
                taps = {}
                ctx["oracle"].forward(spec[:3], taps)
                got = ctx["em"].tap(x[:3], name).cpu().numpy().reshape(taps[name].shape)
                assert _rel(got, taps[name]) < REL_TOL, (front, block, mid, pair, name)
    finally:
        ctx["em"].set_option("fuse_chain", 1)
        ctx["em"].set_option("fuse_se4", 1)
        ctx["em"].set_option("fuse_pair", 1)
        ctx["em"].set_option("fuse_front", 1)
        ctx["em"].set_option("fuse_block", 2)
        ctx["em"].set_option("fuse_mid", 1)
        ctx["em"].set_option("fuse_walk", 1)
        ctx["em"].set_option("fuse_back", 1)
        ctx["em"].set_option("fuse_stem", 1)
        ctx["em"].set_option("fuse_gap", 1)


def test_stride1_big_image_blocks_rows_never_interact(ctx):
    """The stride-1 big-image blocks under the default options (2b on mbconv_mid_kernel, 3b on the front + back pair): depthwise output,
    gate and block output against the oracle for a ragged batch; rows never interact (any sub-batch, any order: bit-identical); silent
    and loud clips at north_star's tolerance."""
    em = ctx["em"]
    rng = np.random.default_rng(33)
    spec = _spec(rng, 37)
    spec[5] = 0.0
    spec[6] = (rng.integers(500, 671, size=(49, 40)) * np.float32(10 / 256))
    x = torch.from_numpy(spec).to(ctx["dev"])
    taps = {}
    ctx["oracle"].forward(spec, taps)
    ordinary = [i for i in range(37) if i not in (5, 6)]
    full = {}
    for name in ("block2b_dw", "block2b_gate", "block2b", "block3b_dw", "block3b_gate", "block3b"):
        got = em.tap(x, name)
        full[name] = got
        g = got.cpu().numpy().reshape(taps[name].shape)
        assert _rel(g[ordinary], taps[name][ordinary]) < REL_TOL, name
        assert _rel(g, taps[name]) < 1e-3, name
        assert _within(g[ordinary], taps[name][ordinary]), name
    for b in (1, 2, 3, 4, 7, 36):
        for name in ("block2b", "block3b_dw", "block3b_gate", "block3b"):
            assert torch.equal(em.tap(x[:b], name), full[name].reshape(37, -1)[:b].reshape(-1)), (b, name)
    perm = torch.randperm(37, device=ctx["dev"])
    for name in ("block2b", "block3b"):
        assert torch.equal(em.tap(x[perm], name).reshape(37, -1), full[name].reshape(37, -1)[perm]), name


def test_depth_fused_chain_is_bit_identical_to_the_single_block_kernels(ctx):
    """mbconv_chain_kernel (blocks 4b..6a in one launch, activations in LDS, residual in registers) and mbconv_pair_chain_kernel (6b..7a in
    one paired launch, all projection tiles exchanged and finished by both halves) perform the same operations in the same order as one
    whole-block launch per block: embeddings and every block output inside the chains are bit-identical, for full, ragged and
    multi-round batches."""
    rng = np.random.default_rng(21)
    spec = _spec(rng, 1024)
    x = torch.from_numpy(spec).to(ctx["dev"])
    em = ctx["em"]
    assert em.get_option("fuse_chain") == 1
    try:
        got = {b: em.forward(x[:b]).clone() for b in (1024, 1023, 37, 9, 8, 7, 6, 5, 4, 3, 1)}
        taps = {n: em.tap(x[:9], n).clone() for n in ("block4b", "block4c", "block5a", "block5b", "block5c", "block6a", "block5b_dw", "block5c_gate", "block6a_dw",
                                                      "block6b", "block6c", "block6d", "block7a", "block6c_dw", "block7a_gate")}
        gap = em.tap(x[:9], "gap").clone()                   # pooled features out of the paired chain's fused top-conv phase
        em.set_option("fuse_top", 0)
        assert torch.equal(em.tap(x[:9], "gap"), gap)          # (a tap runs the stand-alone top conv anyway; the forwards below compare the fused phase)
        for b, e in got.items():
            assert torch.equal(em.forward(x[:b]), e), ("fuse_top", b)
        em.set_option("fuse_top", 1)
        for mode in (0, 2, 3):             # no chain / only the 4x3-image chain / only the paired 2x2-image chain
            em.set_option("fuse_chain", mode)
            for b, e in got.items():
                assert torch.equal(em.forward(x[:b]), e), (mode, b)
            for n, t in taps.items():
                assert torch.equal(em.tap(x[:9], n), t), (mode, n)
    finally:
        em.set_option("fuse_chain", 1)
    ref = ctx["oracle"].forward(spec[:16]).numpy()
    assert _rel(got[1024][:16].cpu().numpy(), ref) < REL_TOL
    # handles of at most 512 clips give the 4x3-image workgroups 2 clips (24 of 32 rows): the other instantiation of the chain
    from multilingual_kws_amd.embedding_model import EmbeddingModel
    em2 = EmbeddingModel(ctx["blob"], max_batch=512)
    try:
        got2 = {b: em2.forward(x[:b]).clone() for b in (512, 511, 37, 5, 4, 2, 1)}
        taps2 = {n: em2.tap(x[:9], n).clone() for n in ("block4c", "block5a", "block5c", "block6a", "block6b", "block6d", "block7a")}
        em2.set_option("fuse_top", 0)
        for b, e in got2.items():
            assert torch.equal(em2.forward(x[:b]), e), ("fuse_top", b)
        em2.set_option("fuse_top", 1)
        for mode in (0, 2, 3):
            em2.set_option("fuse_chain", mode)
            for b, e in got2.items():
                assert torch.equal(em2.forward(x[:b]), e), (mode, b)
            for n, t in taps2.items():
                assert torch.equal(em2.tap(x[:9], n), t), (mode, n)
        assert _rel(got2[512][:16].cpu().numpy(), ref) < REL_TOL
    finally:
        em2.close()


def _default_launch_sequences(blob, big, dev):
    """{"max_batch<N>_B<n>": [[stage, kernel], ...]}: the launches of one forward pass, as mkws_embed_profile names them, for default-option
    handles of 1, 2, 32 and 256 clips at their full batch and for `big` (the module's 1024-clip handle) at its full batch and at 5 clips."""
    from multilingual_kws_amd.embedding_model import EmbeddingModel
    x = torch.from_numpy(_spec(np.random.default_rng(8), big.max_batch)).to(dev)
    seqs = {}
    for max_batch in (1, 2, 32, 256):
        em = EmbeddingModel(blob, max_batch=max_batch)
        seqs[f"max_batch{max_batch}_B{max_batch}"] = [[s, k] for s, k, _ in em.profile(x[:max_batch], reps=1)]
        em.close()
    for b in (big.max_batch, 5):
        seqs[f"max_batch{big.max_batch}_B{b}"] = [[s, k] for s, k, _ in big.profile(x[:b], reps=1)]
    return seqs


def test_default_launch_sequences(ctx, golden_dir):
    """The plan a default-option handle runs is part of the product: the (stage, kernel) sequence of one forward pass, per handle class, is
    the recorded one (tests/golden/embed_launch_sequences.json, written from this function's helper on an MI355X).  A change of routing,
    of a launcher's template choice or of a default shows here as the first differing launch."""
    if torch.cuda.get_device_properties(ctx["dev"]).multi_processor_count != 256:
        pytest.skip("the recorded sequences are those of a 256-CU device (block_mt43 and pair_mt follow the CU count)")
    if ctx["em"].get_option("fuse_pair") != 1:
        pytest.skip("this device's dispatch order failed the probe at create: the paired / cluster kernels are not in the plan")
    want = json.load(open(os.path.join(golden_dir, "embed_launch_sequences.json")))
    got = _default_launch_sequences(ctx["blob"], ctx["em"], ctx["dev"])
    assert sorted(got) == sorted(want)
    for key in want:
        for i, (g, w) in enumerate(zip(got[key], want[key])):
            assert g == w, (key, i, g, w)
        assert len(got[key]) == len(want[key]), (key, len(got[key]), len(want[key]))


def test_golden_embedding_on_device(ctx, golden_dir):
    from multilingual_kws_amd import synth
    from multilingual_kws_amd.frontend import Frontend
    G = json.load(open(os.path.join(golden_dir, "embedding_golden.json")))
    audio = torch.from_numpy(synth.clips_float32(4)).to(ctx["dev"])
    emb = ctx["em"].forward(Frontend().forward(audio)).cpu().numpy()
    assert np.allclose(emb[:, :8], np.asarray(G["embedding_first8"]), rtol=1e-3, atol=1e-5)
    assert np.allclose(np.linalg.norm(emb, axis=1), G["embedding_l2"], rtol=1e-4)
    assert [int(r.argmax()) for r in emb] == G["embedding_argmax"]


def test_ragged_batch_sizes_and_row_masks(ctx):
    """M = B*H*W is rarely a multiple of the 128-row GEMM tile: every B must give the same rows."""
    rng = np.random.default_rng(1)
    spec = _spec(rng, 37)
    x = torch.from_numpy(spec).to(ctx["dev"])
    full = ctx["em"].forward(x)
    ref = ctx["oracle"].forward(spec).numpy()
    assert _rel(full.cpu().numpy(), ref) < REL_TOL
    for b in (1, 2, 3, 7, 16, 33):
        assert torch.equal(ctx["em"].forward(x[:b]), full[:b]), b      # bit-identical: rows never interact
    assert ctx["em"].forward(x[:0]).shape == (0, 1024)


def test_full_batch_properties(ctx):
    """BASELINE size (B=1024): EVERY row against the oracle (round 5: the PyTorch-CPU oracle embeds 128 clips in 0.1 s, there is no reason for a
    subset), batch-composition invariance and determinism on all."""
    rng = np.random.default_rng(2)
    spec = _spec(rng, 1024)
    x = torch.from_numpy(spec).to(ctx["dev"])
    emb = ctx["em"].forward(x)
    got = emb.cpu().numpy()
    ref = np.concatenate([ctx["oracle"].forward(spec[s:s + 128]).numpy() for s in range(0, 1024, 128)])
    assert _rel(got, ref) < REL_TOL
    assert np.abs(got - ref).max(axis=1).max() < REL_TOL * np.abs(ref).max()             # no single row off, whatever its workgroup / pair half
    # 1e-3 relative, every one of the 1 048 576 elements.  The floor for elements next to zero is 2e-5 max|b| against the fp32 PyTorch-CPU oracle --
    # that oracle is itself 1.0e-5 max|b| away from its own fp64 run (tools/se4_accuracy.py: GPU 0.8e-5, fp32 oracle 1.0e-5 from fp64), so two fp32
    # results cannot be held closer than that to each other -- and the literal 1e-5 against the fp64 oracle, on the first 256 clips (fp64 on the CPU
    # costs ~0.1 s per clip)
    assert _within(got, ref, floor=2e-5)
    from oracle.efficientnet_oracle import EmbeddingOracle
    ref64 = np.concatenate([EmbeddingOracle(ctx["blob"], dtype=torch.float64).forward(spec[s:s + 128]).numpy() for s in range(0, 256, 128)])
    assert _within(got[:256].astype(np.float64), ref64.astype(np.float64))
    assert np.array_equal(got.argmax(1), ref.argmax(1))
    perm = torch.randperm(1024, device=ctx["dev"])
    assert torch.equal(ctx["em"].forward(x[perm]), emb[perm])
    assert torch.equal(ctx["em"].forward(x), emb)
    assert torch.isfinite(emb).all()
    big = torch.cat([x, x[:100]])                                       # B > max_batch is chunked by the host wrapper
    assert torch.equal(ctx["em"].forward(big)[1024:], emb[:100])
    for b in (257, 300, 777):          # persistent stem workgroups with unequal clip counts (some walk one clip more than others)
        assert torch.equal(ctx["em"].forward(x[:b]), emb[:b]), b


def test_uncalibrated_weights_and_bad_blobs(ctx):
    """A second weight set (raw random BN statistics) and the error contract of mkws_embed_create."""
    from multilingual_kws_amd import weights
    from multilingual_kws_amd._lib import MkwsError
    from multilingual_kws_amd.embedding_model import EmbeddingModel
    from oracle.efficientnet_oracle import EmbeddingOracle
    blob = weights.synthetic_blob(seed=7, calibrate=False)
    spec = _spec(np.random.default_rng(3), 3)
    em = EmbeddingModel(blob, max_batch=4)
    assert _rel(em.forward(torch.from_numpy(spec).to(ctx["dev"])).cpu().numpy(), EmbeddingOracle(blob).forward(spec).numpy()) < REL_TOL
    with pytest.raises(MkwsError):
        em.forward(torch.zeros((2, 49, 40), device=ctx["dev"]), out=None) if False else EmbeddingModel(blob[:-1], max_batch=4)
    bad = blob.copy(); bad[1000] = np.nan
    with pytest.raises(MkwsError):
        EmbeddingModel(bad, max_batch=4)
    with pytest.raises(ValueError):
        em.forward(torch.zeros((2, 48, 40), device=ctx["dev"]))


def test_weight_container_roundtrip(ctx, tmp_path):
    from multilingual_kws_amd import weights
    weights.save(str(tmp_path / "w"), ctx["blob"])
    assert np.array_equal(weights.load(str(tmp_path / "w")), ctx["blob"])
    named = {t["name"]: ctx["blob"][t["offset"]:t["offset"] + t["count"]].reshape(t["shape"]) for t in weights.manifest()}
    assert np.array_equal(weights.from_named_tensors(named), ctx["blob"])


def test_small_batch_handle_plan(ctx):
    """A small-batch handle (2-clip workgroups / 4-clip pairs instead of 4 / 8): same numbers within fp32 rounding as the
    1024-clip handle, bit-identical across the batch sizes of that handle."""
    from multilingual_kws_amd.embedding_model import EmbeddingModel
    spec = _spec(np.random.default_rng(21), 8)
    x = torch.from_numpy(spec).to(ctx["dev"])
    small = EmbeddingModel(ctx["blob"], max_batch=8)
    out = small.forward(x)
    assert _rel(out.cpu().numpy(), ctx["oracle"].forward(spec).numpy()) < REL_TOL
    assert _rel(out.cpu().numpy(), ctx["em"].forward(x).cpu().numpy()) < REL_TOL
    for b in (1, 3, 5):
        assert torch.equal(small.forward(x[:b]), out[:b]), b


def test_mid_batch_handle_plan(ctx):
    """A 512-clip handle (BASELINE configs[3]) keeps the whole-block kernels but pairs 4 clips instead of 8 (2x2 images) and
    gives a workgroup 2 clips instead of 4 (4x3 images), so that every CU still gets a workgroup: taps of the paired blocks and the embedding against the oracle, batch-size invariance, B = 512."""
    from multilingual_kws_amd.embedding_model import EmbeddingModel
    rng = np.random.default_rng(22)
    spec = _spec(rng, 512)
    x = torch.from_numpy(spec).to(ctx["dev"])
    mid = EmbeddingModel(ctx["blob"], max_batch=512)
    out = mid.forward(x)
    idx = np.arange(0, 512, 41)
    ref = ctx["oracle"].forward(spec[idx]).numpy()
    assert torch.isfinite(out).all() and _rel(out[idx].cpu().numpy(), ref) < REL_TOL
    taps = {}
    ctx["oracle"].forward(spec[:5], taps)
    for name in ("block4b", "block4c_dw", "block5a", "block5b_gate", "block5c", "block6a_dw", "block6a",        # 2 clips per workgroup
                 "block6b_dw", "block6b_gate", "block6b", "block6d", "block7a_gate", "block7a"):              # 4 clips per pair
        got = mid.tap(x[:5], name).cpu().numpy().reshape(taps[name].shape)
        assert _rel(got, taps[name]) < REL_TOL, name
    for b in (1, 3, 4, 5, 37):
        assert torch.equal(mid.forward(x[:b]), out[:b]), b


def test_whole_block_plan_replays_in_a_hip_graph(ctx):
    """The paired whole-block kernel hands partial sums between two workgroups through flags in global memory; the consumer
    resets them, so a captured launch (fixed kernel arguments, no host-side epoch) must replay any number of times."""
    rng = np.random.default_rng(5)
    xs = [torch.from_numpy(_spec(rng, 21)).to(ctx["dev"]) for _ in range(3)]      # 21 clips: two full pairs + a ragged one
    refs = [ctx["em"].forward(x).clone() for x in xs]
    static_in = xs[0].clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ctx["em"].forward(static_in)
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = ctx["em"].forward(static_in)
    for k in (0, 1, 2, 1, 0):
        static_in.copy_(xs[k])
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, refs[k]), k


@pytest.mark.parametrize("chain", [1, 2])          # 1: the paired CHAIN kernel (6b..7a in one launch); 2: one paired launch per block
@pytest.mark.parametrize("fault", [1, 2])
def test_failed_pair_exchange_degrades_instead_of_poisoning(ctx, fault, chain):
    """include/mkws.h, "Failure contract of the paired whole-block kernel": when the two halves of a pair land on different
    XCDs (fault 1, forced through the test hook) or a half never arrives (fault 2: the other times out), the failing forward is
    NaN-poisoned, the NEXT call returns MKWS_ERR_EXCHANGE having moved the handle to the single-workgroup kernel, and the
    repeated call is correct -- for good, with no stale flag left behind."""
    from multilingual_kws_amd import _lib
    from multilingual_kws_amd.embedding_model import EmbeddingModel
    spec = _spec(np.random.default_rng(40 + fault), 24)
    x = torch.from_numpy(spec).to(ctx["dev"])
    ref = ctx["oracle"].forward(spec).numpy()
    em = EmbeddingModel(ctx["blob"], max_batch=1024)
    if em.get_option("fuse_pair") != 1:
        pytest.skip("this device's dispatch order failed the probe at create: the paired kernel is not in use")
    em.set_option("fuse_chain", chain)
    assert _rel(em.forward(x).cpu().numpy(), ref) < REL_TOL and em.get_option("pair_degraded") == 0
    em.set_option("pair_fault", fault)
    poisoned = em.forward(x)
    torch.cuda.synchronize()
    assert torch.isnan(poisoned).all()                                   # safe-fail: never a plausible wrong number (the last layer reads the error word)
    em.set_option("pair_fault", 0)
    emb = torch.empty((24, 1024), device=ctx["dev"])
    rc = em.L.mkws_embed_forward(em.h, x.data_ptr(), 24, emb.data_ptr(), _lib.current_stream_ptr())
    assert rc == _lib.MKWS_ERR_EXCHANGE and b"repeat the call" in em.L.mkws_last_error()
    assert em.get_option("fuse_pair") == 0 and em.get_option("pair_degraded") == 1
    for _ in range(2):                                                   # the retry, and the call after it
        out = em.forward(x)
        assert torch.isfinite(out).all() and _rel(out.cpu().numpy(), ref) < REL_TOL
    # the Python wrapper retries by itself (with a warning) when it is the one that meets the error code
    em2 = EmbeddingModel(ctx["blob"], max_batch=1024)
    em2.set_option("fuse_chain", chain)
    em2.set_option("pair_fault", fault)
    em2.forward(x)
    torch.cuda.synchronize()
    with pytest.warns(RuntimeWarning, match="NaN-poisoned"):
        out = em2.forward(x)
    assert _rel(out.cpu().numpy(), ref) < REL_TOL and em2.get_option("pair_degraded") == 1
    # re-arming the paired kernel after the reset works: flags and the sticky word were cleared in stream order
    em2.set_option("fuse_pair", 1)
    assert _rel(em2.forward(x).cpu().numpy(), ref) < REL_TOL and em2.get_option("pair_degraded") == 1
    # the numpy-facing API (predict) has synchronised for its device-to-host copy and looks at the handle before it returns: the poisoned
    # batch never reaches the caller
    em3 = EmbeddingModel(ctx["blob"], max_batch=1024)
    em3.set_option("fuse_chain", chain)
    em3.set_option("pair_fault", fault)
    with pytest.warns(RuntimeWarning, match="repeating it"):
        out = em3.predict(spec[..., None])
    assert np.isfinite(out).all() and _rel(out, ref) < REL_TOL
    assert em3.get_option("pair_degraded") == 1 and em3.get_option("fuse_pair") == 0 and em3.get_option("exchange_error") == 0


@pytest.mark.parametrize("plan", ["default", "multi-kernel", "no-cluster"])
@pytest.mark.parametrize("max_batch", [1, 2, 5, 32, 256])
def test_serving_handle_plans(ctx, max_batch, plan):
    """The handles bench.py's streaming config builds (BASELINE configs[4]: max_batch 1 for the latency leg, 256 for throughput)
    against the oracle, with batch-size invariance inside the handle -- on the shipped plan (whole-block kernels for every handle
    size since round 3) and on the multi-kernel path (split-K projections, separate SE launches) that small handles used before."""
    from multilingual_kws_amd.embedding_model import EmbeddingModel
    n = min(max_batch, 40)
    spec = _spec(np.random.default_rng(60 + max_batch), n)
    x = torch.from_numpy(spec).to(ctx["dev"])
    em = EmbeddingModel(ctx["blob"], max_batch=max_batch)
    if plan == "multi-kernel":
        for k in ("fuse_block", "fuse_mid", "fuse_back", "fuse_pair", "fuse_cluster"):
            em.set_option(k, 0)
    elif plan == "no-cluster":
        em.set_option("fuse_cluster", 0)
    else:
        # (one-clip handles run blocks 2b / 3a / 4a on the split front / back kernels: several CUs per clip instead of one workgroup, round 6)
        assert em.get_option("fuse_block") == 2 and em.get_option("fuse_mid") == (0 if max_batch == 1 else 1)
        # live-serving handles (<= 32 clips) run the tiny-image blocks on the 6-way cluster kernel (when the dispatch probe passed)
        assert em.get_option("fuse_cluster") == (1 if max_batch <= 32 and em.get_option("fuse_pair") else 0)
    out = em.forward(x)
    ref = ctx["oracle"].forward(spec).numpy()
    assert _rel(out.cpu().numpy(), ref) < REL_TOL and np.array_equal(out.cpu().numpy().argmax(1), ref.argmax(1))
    for b in sorted({1, n // 2, n - 1} - {0}):
        assert torch.equal(em.forward(x[:b]), out[:b]), b
    if max_batch <= 4:
        # round 6: the dense tail (and, for a one-clip handle, the top conv + pool) of live-serving handles runs on gemv_kernel: one launch per
        # layer, K split inside the workgroup.  Against the MFMA GEMM + split-K fold it replaces: another summation order, fp32 round-off
        assert em.get_option("fuse_gemv") == 1
        xs = x[:max_batch]
        for name in ("gap", "dense", "dense_1", "dense_2"):
            t = {}
            ctx["oracle"].forward(spec[:max_batch], t)
            assert _rel(em.tap(xs, name).cpu().numpy().reshape(t[name].shape), t[name]) < REL_TOL, name
        em.set_option("fuse_gemv", 0)
        try:
            assert _rel(em.forward(x).cpu().numpy(), out.cpu().numpy()) < 1e-5
        finally:
            em.set_option("fuse_gemv", 1)
    if max_batch == 256:
        if plan not in ("multi-kernel",):
            assert em.get_option("block_tiles") == 1        # round 6: one clip per workgroup of the 4x3-image chain (256 workgroups on 256 CUs, not 128)
        full = _spec(np.random.default_rng(7), 256)
        xf = torch.from_numpy(full).to(ctx["dev"])
        of = em.forward(xf)
        idx = np.arange(0, 256, 23)
        assert _rel(of[idx].cpu().numpy(), ctx["oracle"].forward(full[idx]).numpy()) < REL_TOL
        assert torch.equal(em.forward(xf[:n]), of[:n])
        if plan not in ("multi-kernel",):
            # every workgroup shape of the 4x3-image kernels on the same handle: depth-fused chain and single-block launches, against each other
            # at fp32 round-off (another tile shape = another plan) and against the oracle
            try:
                for tiles in (2, 3, 1):
                    em.set_option("block_tiles", tiles)
                    for chain in (1, 0):
                        em.set_option("fuse_chain", chain)
                        o2 = em.forward(xf)
                        assert _rel(o2.cpu().numpy(), of.cpu().numpy()) < 1e-5, (tiles, chain)
                        for name in ("block4c", "block5b_dw", "block5b_gate", "block6a"):
                            t2 = {}
                            ctx["oracle"].forward(full[:5], t2)
                            assert _rel(em.tap(xf[:5], name).cpu().numpy().reshape(t2[name].shape), t2[name]) < REL_TOL, (tiles, chain, name)
            finally:
                em.set_option("block_tiles", 0)
                em.set_option("fuse_chain", 1)


def test_cluster_kernel_taps_and_failure_contract(ctx):
    """mbconv_cluster_kernel (small-batch handles: six workgroups share one 16-row tile and split the expanded channels): inner taps of
    every block it runs against the oracle, ragged clip counts (1 clip per cluster on 4x3 images, 4 on 2x2), graph-free repeat calls
    (generation flags), and the shared failure contract (forced XCC mismatch / missing member -> NaN, MKWS_ERR_EXCHANGE, degraded)."""
    from multilingual_kws_amd import _lib
    from multilingual_kws_amd.embedding_model import EmbeddingModel
    spec = _spec(np.random.default_rng(77), 7)
    x = torch.from_numpy(spec).to(ctx["dev"])
    em = EmbeddingModel(ctx["blob"], max_batch=7)
    if em.get_option("fuse_cluster") != 1:
        pytest.skip("dispatch probe failed on this device: the cluster kernel is not in use")
    taps = {}
    ref = ctx["oracle"].forward(spec, taps).numpy()
    for name in ("block4b_dw", "block4b_gate", "block4b", "block4c", "block5a_dw", "block5a", "block5b_gate", "block5b", "block5c", "block6a_dw", "block6a_gate",
                 "block6a", "block6b_dw", "block6b_gate", "block6b", "block6c", "block6d", "block7a_dw", "block7a_gate", "block7a"):
        got = em.tap(x, name).cpu().numpy().reshape(taps[name].shape)
        assert _rel(got, taps[name]) < REL_TOL, name
    out = em.forward(x)
    assert _rel(out.cpu().numpy(), ref) < REL_TOL
    for b in (1, 2, 3, 4, 5, 6):
        assert torch.equal(em.forward(x[:b]), out[:b]), b                     # and 20+ launches per call exercise the generation flags
    for fault in (1, 2):
        emf = EmbeddingModel(ctx["blob"], max_batch=7)
        emf.set_option("pair_fault", fault)
        bad = emf.forward(x)
        torch.cuda.synchronize()
        assert torch.isnan(bad).all()
        emf.set_option("pair_fault", 0)
        emb = torch.empty((7, 1024), device=ctx["dev"])
        rc = emf.L.mkws_embed_forward(emf.h, x.data_ptr(), 7, emb.data_ptr(), _lib.current_stream_ptr())
        assert rc == _lib.MKWS_ERR_EXCHANGE and emf.get_option("fuse_cluster") == 0 and emf.get_option("fuse_pair") == 0
        again = emf.forward(x)
        assert torch.isfinite(again).all() and _rel(again.cpu().numpy(), ref) < REL_TOL
        emf.set_option("fuse_cluster", 1)                                      # re-armed after the reset: flags were cleared in stream order
        assert _rel(emf.forward(x).cpu().numpy(), ref) < REL_TOL
    big = EmbeddingModel(ctx["blob"], max_batch=128)
    with pytest.raises(_lib.MkwsError):
        big.set_option("fuse_cluster", 1)                                      # no exchange buffers above 64 clips


def test_cluster_chain_plan_of_one_clip_handles(ctx):
    """mbconv_cluster_chain_kernel (round 6): a live window's blocks 4b .. 7a as ONE launch -- the members of all ten blocks request their
    weights together and a block starts when the previous one has published its output (write-through stores, generation words).  Same
    arithmetic in the same order as the launch-by-launch cluster plan: bit-identical to it, on many windows in a row (stale-line / generation
    bugs show as a mismatch on a later call), replayed from a hipGraph, against the oracle, and the shared failure contract."""
    from multilingual_kws_amd import _lib
    from multilingual_kws_amd.embedding_model import EmbeddingModel
    rng = np.random.default_rng(91)
    specs = _spec(rng, 24)
    em = EmbeddingModel(ctx["blob"], max_batch=1)
    if em.get_option("fuse_cluster") != 1:
        pytest.skip("dispatch probe failed on this device: the cluster kernels are not in use")
    assert em.get_option("fuse_cluster_chain") == 1
    ref = ctx["oracle"].forward(specs).numpy()
    xs = torch.from_numpy(specs).to(ctx["dev"])
    chained = torch.stack([em.forward(xs[i:i + 1])[0].clone() for i in range(24)])
    em.set_option("fuse_cluster_chain", 0)
    single = torch.stack([em.forward(xs[i:i + 1])[0].clone() for i in range(24)])
    em.set_option("fuse_cluster_chain", 1)
    assert torch.equal(chained, single)
    assert _rel(chained.cpu().numpy(), ref) < REL_TOL and np.array_equal(chained.cpu().numpy().argmax(1), ref.argmax(1))
    # alternating inputs, back to back without a synchronisation: window i must never see window i - 1's activations
    for rep in range(50):
        i = rep % 24
        assert torch.equal(em.forward(xs[i:i + 1])[0], chained[i]), rep
    # taps inside the chain's range run launch by launch and agree with the oracle; the forward after them is unchanged
    taps = {}
    ctx["oracle"].forward(specs[:1], taps)
    for name in ("block4b", "block5b_gate", "block6a", "block6c_dw", "block7a"):
        assert _rel(em.tap(xs[:1], name).cpu().numpy().reshape(taps[name].shape), taps[name]) < REL_TOL, name
    assert torch.equal(em.forward(xs[:1])[0], chained[0])
    # hipGraph replay (the serving path): generation words, no per-launch arguments
    xin = xs[3:4].clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        em.forward(xin)
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out_g = em.forward(xin)
    for i in (3, 7, 11, 3):
        xin.copy_(xs[i:i + 1])
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out_g[0], chained[i]), i
    # a larger handle does not take the option
    with pytest.raises(_lib.MkwsError):
        EmbeddingModel(ctx["blob"], max_batch=2).set_option("fuse_cluster_chain", 1)
    # three handles at once, a stream each (uneven load on the L2s: the first build of the kernel let blocks on different XCDs share one
    # exchange slot and returned silently wrong windows here, never alone): every window identical to the lone result, nothing degraded
    others = [em] + [EmbeddingModel(ctx["blob"], max_batch=1) for _ in range(2)]
    streams = [torch.cuda.Stream() for _ in others]
    torch.cuda.synchronize()
    outs = [[torch.empty((1, 1024), device=ctx["dev"]) for _ in range(60)] for _ in others]
    for w in range(60):
        for k, (e, st) in enumerate(zip(others, streams)):
            with torch.cuda.stream(st):
                e.forward(xs[(w + 5 * k) % 24:(w + 5 * k) % 24 + 1], out=outs[k][w])
    torch.cuda.synchronize()
    for k, e in enumerate(others):
        assert e.get_option("pair_degraded") == 0 and e.get_option("fuse_cluster_chain") == 1
        for w in range(60):
            assert torch.equal(outs[k][w][0], chained[(w + 5 * k) % 24]), (k, w)
    # failure contract: a member that never arrives (fault 2) / a wrong XCC id (fault 1) poison the window, the next call reports and degrades
    for fault in (1, 2):
        emf = EmbeddingModel(ctx["blob"], max_batch=1)
        emf.set_option("pair_fault", fault)
        bad = emf.forward(xs[:1])
        torch.cuda.synchronize()
        assert torch.isnan(bad).all()
        emf.set_option("pair_fault", 0)
        emb = torch.empty((1, 1024), device=ctx["dev"])
        rc = emf.L.mkws_embed_forward(emf.h, xs[:1].data_ptr(), 1, emb.data_ptr(), _lib.current_stream_ptr())
        assert rc == _lib.MKWS_ERR_EXCHANGE and emf.get_option("fuse_cluster_chain") == 0 and emf.get_option("fuse_cluster") == 0
        again = emf.forward(xs[:1])
        assert torch.isfinite(again).all() and _rel(again.cpu().numpy(), ref[:1]) < REL_TOL
